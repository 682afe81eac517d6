// odom.hip — odometry driver around the GICP core (include/ddlo_odom.h;
// SURVEY.md §8(f) rank 1, device voxel filter = rank 3).
//
// Restates the registration half of OdomNode (reference
// dynamic_direct_lidar_odometry/src/odometry/odom.cc) with every point set
// on the device:
//   icpCB                 :614-729   process()
//   preprocessPoints      :442-478   crop box + voxel filter (preprocess.hip)
//   computeSpaciousness   :981-1001  device ranges + sort, host low-pass
//   setAdaptiveParams     :1156-1178
//   initializeInputTarget :480-516
//   setInputSources       :518-532   one device cloud shared by S2S and S2M
//   scanMatching          :745-851   S2S, propagateS2S, cov reuse, swap,
//                                    getSubmapKeyframes, S2M, propagateS2M
//   transformScans        :941-947   device transform to the world frame
//   applySegmentation     :853-918   process_dynamic: world-frame scan (device),
//                                    residual image, segmentation, objects, the
//                                    caller's verdict; a new keyframe's cloud
//                                    is the scan without the non-static objects
//   updateKeyframes       :1067-1154 keyframe decision; the keyframe cloud
//                                    (submap voxel filter) and its k-NN
//                                    covariances stay on the device
//   getSubmapKeyframes    :1215-1315 k nearest + convex-hull + concave-hull
//                                    keyframes; the submap cloud is the
//                                    device concatenation of the keyframes'
//                                    points and covariances (no host copies)
// Deliberate differences, all where the reference reads unsynchronised or
// out-of-range data: the spaciousness metric is computed before the
// adaptive threshold reads it (the reference starts it on a detached thread
// right before, :656-660) and over the scan's n points (its loop reads one
// past the end, :986).
#include <hip/hip_runtime.h>

#include <chrono>
#include <cstdio>

#include <algorithm>
#include <array>
#include <cfloat>
#include <cmath>
#include <cstring>
#include <map>
#include <memory>
#include <queue>
#include <vector>

#include "../../include/ddlo_gicp.h"
#include "../../include/ddlo_odom.h"
#include "../../include/ddlo_track.h"
#include "gicp_types.hpp"
#include "launch.hpp"
#include "runtime.hpp"
#include "devknobs.hpp"
#include "seg_internal.hpp"
#include "odom_internal.hpp"
#include "track_internal.hpp"

namespace {

using namespace ddlo;
using namespace ddlo::rt;

// ---- small host math (float like the reference's Matrix4f / Quaternionf) ----
void mat4_identity(float* T) {
  for (int i = 0; i < 16; ++i) T[i] = (i % 5 == 0) ? 1.f : 0.f;
}
void mat4_mul(const float* A, const float* B, float* C) {  // C = A * B, row-major
  float R[16];
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c)
      R[4 * r + c] = ((A[4 * r] * B[c] + A[4 * r + 1] * B[4 + c]) + A[4 * r + 2] * B[8 + c]) + A[4 * r + 3] * B[12 + c];
  std::memcpy(C, R, sizeof(R));
}

struct Quatf {
  float x = 0.f, y = 0.f, z = 0.f, w = 1.f;
};

// Eigen::Quaternionf(const Matrix3f&) (quaternionbase_assign_impl), then the
// normalisation of propagateS2M (odom.cc:928-937: double norm, float /=)
Quatf quat_from_R(const float* T) {
  auto m = [&](int r, int c) { return T[4 * r + c]; };
  Quatf q;
  float t = m(0, 0) + m(1, 1) + m(2, 2);
  if (t > 0.f) {
    t = std::sqrt(t + 1.0f);
    q.w = 0.5f * t;
    t = 0.5f / t;
    q.x = (m(2, 1) - m(1, 2)) * t;
    q.y = (m(0, 2) - m(2, 0)) * t;
    q.z = (m(1, 0) - m(0, 1)) * t;
  } else {
    int i = 0;
    if (m(1, 1) > m(0, 0)) i = 1;
    if (m(2, 2) > m(i, i)) i = 2;
    const int j = (i + 1) % 3, k = (j + 1) % 3;
    t = std::sqrt(m(i, i) - m(j, j) - m(k, k) + 1.0f);
    float c[3];
    c[i] = 0.5f * t;
    t = 0.5f / t;
    q.w = (m(k, j) - m(j, k)) * t;
    c[j] = (m(j, i) + m(i, j)) * t;
    c[k] = (m(k, i) + m(i, k)) * t;
    q.x = c[0];
    q.y = c[1];
    q.z = c[2];
  }
  const double norm = std::sqrt(q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z);
  q.w = (float)(q.w / norm);
  q.x = (float)(q.x / norm);
  q.y = (float)(q.y / norm);
  q.z = (float)(q.z / norm);
  return q;
}

Quatf quat_mul(const Quatf& a, const Quatf& b) {
  Quatf r;
  r.w = a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z;
  r.x = a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y;
  r.y = a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z;
  r.z = a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x;
  return r;
}
Quatf quat_inverse(const Quatf& q) {  // Eigen: conjugate / squaredNorm
  const float n2 = q.w * q.w + q.x * q.x + q.y * q.y + q.z * q.z;
  Quatf r;
  r.w = q.w / n2;
  r.x = -q.x / n2;
  r.y = -q.y / n2;
  r.z = -q.z / n2;
  return r;
}

// ---- hulls over the keyframe positions (computeConvexHull / computeConcaveHull) ----
// OdomNode sets both hulls to dimension 3 (odom.cc:87-88), so PCL never
// projects to a plane: pcl::ConvexHull runs qhull in 3-D ("qhull ", no
// joggle; a flat keyframe set is a qhull precision error and an EMPTY hull),
// pcl::ConcaveHull runs qhull's 3-D Delaunay ("qhull d QJ") and keeps the
// alpha shape's boundary triangles.  Both are restated here on the host (a
// few hundred keyframes at most), as the reference runs qhull on its host.
using P3 = std::array<double, 3>;

// vertex set of the 3-D convex hull; empty when the points are coplanar or
// fewer than 4 (qhull: "initial simplex is flat")
std::vector<int> convex_hull(const float* xyz, int n) {
  std::vector<int> out;
  if (n < 4) return out;
  struct F {
    int a, b, c;
    double n[3], d;
    bool alive;
  };
  auto P = [&](int i) { return P3{xyz[3 * i], xyz[3 * i + 1], xyz[3 * i + 2]}; };
  auto make = [&](int a, int b, int cc) {
    const P3 A = P(a), B = P(b), Cc = P(cc);
    const double e1[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, e2[3] = {Cc[0] - A[0], Cc[1] - A[1], Cc[2] - A[2]};
    F f{a, b, cc, {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]}, 0, true};
    const double nn = std::sqrt(f.n[0] * f.n[0] + f.n[1] * f.n[1] + f.n[2] * f.n[2]);
    if (nn > 0)
      for (int k = 0; k < 3; ++k) f.n[k] /= nn;   // unit normal: the visibility test below is a distance
    f.d = f.n[0] * A[0] + f.n[1] * A[1] + f.n[2] * A[2];
    return f;
  };
  double scale = 0;
  for (int i = 0; i < 3 * n; ++i) scale = std::max(scale, (double)std::fabs(xyz[i]));
  scale = std::max(scale, 1e-30);
  const double eps = 1e-12 * scale;   // a point this close to a facet's plane does not see it (qhull: round-off)
  // initial tetrahedron: farthest-apart picks
  int i0 = 0, i1 = -1, i2 = -1, i3 = -1;
  double best = -1;
  for (int i = 1; i < n; ++i) {
    const P3 a = P(i0), b = P(i);
    const double d = (a[0] - b[0]) * (a[0] - b[0]) + (a[1] - b[1]) * (a[1] - b[1]) + (a[2] - b[2]) * (a[2] - b[2]);
    if (d > best) { best = d; i1 = i; }
  }
  best = -1;
  for (int i = 0; i < n; ++i) {
    if (i == i0 || i == i1) continue;
    const P3 A = P(i0), B = P(i1), Cc = P(i);
    const double e1[3] = {B[0] - A[0], B[1] - A[1], B[2] - A[2]}, e2[3] = {Cc[0] - A[0], Cc[1] - A[1], Cc[2] - A[2]};
    const double cx = e1[1] * e2[2] - e1[2] * e2[1], cy = e1[2] * e2[0] - e1[0] * e2[2], cz = e1[0] * e2[1] - e1[1] * e2[0];
    const double a2 = cx * cx + cy * cy + cz * cz;
    if (a2 > best) { best = a2; i2 = i; }
  }
  if (i2 < 0 || !(best > 0)) return out;   // collinear
  best = -1;
  const F base = make(i0, i1, i2);
  const double bn = 1.0;
  for (int i = 0; i < n; ++i) {
    if (i == i0 || i == i1 || i == i2) continue;
    const P3 p = P(i);
    const double sd = std::fabs(base.n[0] * p[0] + base.n[1] * p[1] + base.n[2] * p[2] - base.d);
    if (sd > best) { best = sd; i3 = i; }
  }
  // qhull's flat-simplex test is at round-off level: coplanar within ~1e-13 of the extent
  if (!(bn > 0) || i3 < 0 || best / bn <= 1e-13 * scale) return out;
  std::vector<F> fs;
  auto add_oriented = [&](int a, int b, int cc, int inside) {
    F f = make(a, b, cc);
    const P3 q = P(inside);
    if (f.n[0] * q[0] + f.n[1] * q[1] + f.n[2] * q[2] - f.d > 0) f = make(a, cc, b);
    fs.push_back(f);
  };
  add_oriented(i0, i1, i2, i3);
  add_oriented(i0, i1, i3, i2);
  add_oriented(i0, i2, i3, i1);
  add_oriented(i1, i2, i3, i0);
  for (int i = 0; i < n; ++i) {
    if (i == i0 || i == i1 || i == i2 || i == i3) continue;
    const P3 p = P(i);
    std::vector<std::pair<int, int>> edges;
    bool any = false;
    for (auto& f : fs) {
      if (!f.alive) continue;
      if (f.n[0] * p[0] + f.n[1] * p[1] + f.n[2] * p[2] - f.d > eps) {
        f.alive = false;
        any = true;
        edges.push_back({f.a, f.b});
        edges.push_back({f.b, f.c});
        edges.push_back({f.c, f.a});
      }
    }
    if (!any) continue;
    // horizon: directed edges whose reverse was not removed
    for (const auto& e : edges) {
      bool twin = false;
      for (const auto& g : edges)
        if (g.first == e.second && g.second == e.first) { twin = true; break; }
      if (!twin) fs.push_back(make(e.first, e.second, i));
    }
  }
  std::vector<char> on(n, 0);
  for (const auto& f : fs)
    if (f.alive) on[f.a] = on[f.b] = on[f.c] = 1;
  for (int i = 0; i < n; ++i)
    if (on[i]) out.push_back(i);
  return out;
}

// ---- 3-D Delaunay (Bowyer-Watson, long double predicates) ----
using LD = long double;
struct Tet {
  int v[4];
  bool alive;
};

LD det3(LD a, LD b, LD c, LD d, LD e, LD f, LD g, LD h, LD i) { return a * (e * i - f * h) - b * (d * i - f * g) + c * (d * h - e * g); }

// det[b - a; c - a; d - a]
LD orient(const std::vector<std::array<LD, 3>>& p, int a, int b, int c, int d) {
  const auto& A = p[a];
  const auto& B = p[b];
  const auto& C = p[c];
  const auto& D = p[d];
  return det3(B[0] - A[0], B[1] - A[1], B[2] - A[2], C[0] - A[0], C[1] - A[1], C[2] - A[2], D[0] - A[0], D[1] - A[1],
              D[2] - A[2]);
}

// 4x4 lifted determinant; for a positively oriented tetrahedron its sign
// tells whether e lies inside the circumsphere (kInside below)
LD insphere(const std::vector<std::array<LD, 3>>& p, const int* t, int e) {
  LD m[4][4];
  for (int r = 0; r < 4; ++r) {
    const auto& A = p[t[r]];
    const LD x = A[0] - p[e][0], y = A[1] - p[e][1], z = A[2] - p[e][2];
    m[r][0] = x;
    m[r][1] = y;
    m[r][2] = z;
    m[r][3] = x * x + y * y + z * z;
  }
  LD d = 0;
  for (int c = 0; c < 4; ++c) {
    LD sub[9];
    int k = 0;
    for (int r = 1; r < 4; ++r)
      for (int cc = 0; cc < 4; ++cc)
        if (cc != c) sub[k++] = m[r][cc];
    const LD cof = det3(sub[0], sub[1], sub[2], sub[3], sub[4], sub[5], sub[6], sub[7], sub[8]);
    d += ((c & 1) ? -1 : 1) * m[0][c] * cof;
  }
  return d;
}

int inside_sign() {   // the sign insphere() has at the centre of a positive unit tetrahedron
  static const int s = [] {
    std::vector<std::array<LD, 3>> p = {{0, 0, 0}, {1, 0, 0}, {0, 1, 0}, {0, 0, 1}, {0.25L, 0.25L, 0.25L}};
    const int t[4] = {0, 1, 2, 3};
    return insphere(p, t, 4) > 0 ? 1 : -1;
  }();
  return s;
}

// Delaunay tetrahedra of the points (indices into xyz), the enclosing
// tetrahedron's removed.  Input coordinates are demeaned (PCL demeans before
// qhull) and joggled by a deterministic relative 1e-11 (qhull's QJ joggles
// randomly) so that cospherical / coplanar input has a well-defined answer.
std::vector<Tet> delaunay3(const float* xyz, int n, std::vector<std::array<LD, 3>>& p) {
  std::array<LD, 3> c{0, 0, 0};
  for (int i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) c[a] += xyz[3 * i + a];
  for (int a = 0; a < 3; ++a) c[a] /= n;
  LD ext = 0;
  p.assign(n + 4, {0, 0, 0});
  uint64_t rng = 0x9E3779B97F4A7C15ull;
  auto next = [&]() {
    rng ^= rng << 13;
    rng ^= rng >> 7;
    rng ^= rng << 17;
    return (LD)((rng >> 11) * (1.0 / 9007199254740992.0)) - 0.5L;
  };
  for (int i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) {
      p[i][a] = (LD)xyz[3 * i + a] - c[a];
      ext = std::max(ext, std::fabs(p[i][a]));
    }
  ext = std::max(ext, (LD)1e-12);
  for (int i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) p[i][a] += next() * 1e-11L * ext;
  const LD M = 1e4L * ext;
  p[n] = {-M, -M, -M};
  p[n + 1] = {3 * M, -M, -M};
  p[n + 2] = {-M, 3 * M, -M};
  p[n + 3] = {-M, -M, 3 * M};
  std::vector<Tet> T;
  T.push_back({{n, n + 1, n + 2, n + 3}, true});
  if (orient(p, n, n + 1, n + 2, n + 3) < 0) std::swap(T[0].v[2], T[0].v[3]);
  const int ins = inside_sign();
  for (int i = 0; i < n; ++i) {
    std::vector<int> bad;
    for (int t = 0; t < (int)T.size(); ++t)
      if (T[t].alive && insphere(p, T[t].v, i) * ins > 0) bad.push_back(t);
    // cavity boundary: faces of exactly one bad tetrahedron
    std::map<std::array<int, 3>, std::pair<int, std::array<int, 3>>> faces;
    for (int t : bad) {
      T[t].alive = false;
      const int* v = T[t].v;
      const int fidx[4][3] = {{1, 2, 3}, {0, 3, 2}, {0, 1, 3}, {0, 2, 1}};
      for (const auto& f : fidx) {
        std::array<int, 3> o{v[f[0]], v[f[1]], v[f[2]]};
        std::array<int, 3> k = o;
        std::sort(k.begin(), k.end());
        auto it = faces.find(k);
        if (it == faces.end()) faces[k] = {1, o};
        else it->second.first += 1;
      }
    }
    for (const auto& kv : faces) {
      if (kv.second.first != 1) continue;
      const auto& o = kv.second.second;
      Tet nt{{o[0], o[1], o[2], i}, true};
      const LD ov = orient(p, nt.v[0], nt.v[1], nt.v[2], nt.v[3]);
      if (ov == 0) continue;   // degenerate after joggle: drop (never seen)
      if (ov < 0) std::swap(nt.v[0], nt.v[1]);
      T.push_back(nt);
    }
  }
  std::vector<Tet> out;
  for (const auto& t : T)
    if (t.alive && t.v[0] < n && t.v[1] < n && t.v[2] < n && t.v[3] < n) out.push_back(t);
  return out;
}

// circumradius of a tetrahedron (qh_pointdist(vertex, facet->center))
LD tet_radius(const std::vector<std::array<LD, 3>>& p, const Tet& t) {
  const auto& A = p[t.v[0]];
  LD r[3][3], rhs[3];
  for (int k = 0; k < 3; ++k) {
    const auto& B = p[t.v[k + 1]];
    for (int a = 0; a < 3; ++a) r[k][a] = B[a] - A[a];
    rhs[k] = 0.5L * (r[k][0] * r[k][0] + r[k][1] * r[k][1] + r[k][2] * r[k][2]);
  }
  const LD D = det3(r[0][0], r[0][1], r[0][2], r[1][0], r[1][1], r[1][2], r[2][0], r[2][1], r[2][2]);
  if (D == 0) return INFINITY;
  const LD x = det3(rhs[0], r[0][1], r[0][2], rhs[1], r[1][1], r[1][2], rhs[2], r[2][1], r[2][2]) / D;
  const LD y = det3(r[0][0], rhs[0], r[0][2], r[1][0], rhs[1], r[1][2], r[2][0], rhs[2], r[2][2]) / D;
  const LD z = det3(r[0][0], r[0][1], rhs[0], r[1][0], r[1][1], rhs[1], r[2][0], r[2][1], rhs[2]) / D;
  return std::sqrt(x * x + y * y + z * z);
}

// pcl::getCircumcircleRadius (common/impl/common.hpp) of a ridge, whose
// vertices PCL reads as floats of qhull's (demeaned) coordinates: float
// Vector4f norms (Eigen's SSE redux: (x^2 + z^2) + y^2), Heron's formula in double
double tri_radius(const std::vector<std::array<LD, 3>>& p, int a, int b, int c) {
  auto nrm = [&](int i, int j) {
    const float dx = (float)p[j][0] - (float)p[i][0], dy = (float)p[j][1] - (float)p[i][1],
                dz = (float)p[j][2] - (float)p[i][2];
    return (double)std::sqrt((dx * dx + dz * dz) + dy * dy);
  };
  const double p2p1 = nrm(a, b), p3p2 = nrm(b, c), p1p3 = nrm(c, a);
  const double s = (p2p1 + p3p2 + p1p3) / 2.0;
  const double area = std::sqrt(s * (s - p2p1) * (s - p3p2) * (s - p1p3));
  return (p2p1 * p3p2 * p1p3) / (4.0 * area);
}

// Vertex set of pcl::ConcaveHull's 3-D alpha shape (PCL 1.10
// concave_hull.hpp performReconstruction, dim 3): a tetrahedron is "good"
// iff its circumradius <= alpha; a Delaunay triangle is output iff it has a
// side that is not a good tetrahedron (the outside, or a bad one) and its
// circumradius <= alpha (a good tetrahedron's triangles always are);
// setKeepInformation maps the vertices back to input indices.
std::vector<int> concave_hull(const float* xyz, int n, double alpha) {
  std::vector<int> out;
  if (n < 4) return out;
  std::vector<std::array<LD, 3>> p;
  const std::vector<Tet> T = delaunay3(xyz, n, p);
  std::vector<char> good(T.size());
  std::map<std::array<int, 3>, std::array<int, 2>> adj;   // triangle -> its tetrahedra (-1 = outside)
  for (size_t t = 0; t < T.size(); ++t) {
    good[t] = tet_radius(p, T[t]) <= (LD)alpha;
    const int* v = T[t].v;
    const int fidx[4][3] = {{1, 2, 3}, {0, 3, 2}, {0, 1, 3}, {0, 2, 1}};
    for (const auto& f : fidx) {
      std::array<int, 3> k{v[f[0]], v[f[1]], v[f[2]]};
      std::sort(k.begin(), k.end());
      auto it = adj.find(k);
      if (it == adj.end()) adj[k] = {(int)t, -1};
      else it->second[1] = (int)t;
    }
  }
  std::vector<char> on(n, 0);
  for (const auto& kv : adj) {
    const int a = kv.second[0], b = kv.second[1];
    const bool ga = good[a], gb = b >= 0 && good[b];
    if (ga && gb) continue;   // inside the good union
    const auto& f = kv.first;
    if (ga || gb || tri_radius(p, f[0], f[1], f[2]) <= alpha) on[f[0]] = on[f[1]] = on[f[2]] = 1;
  }
  for (int i = 0; i < n; ++i)
    if (on[i]) out.push_back(i);
  return out;
}

// OdomNode::pushSubmapIndices (odom.cc:1180-1213): the k smallest distances
// (max-heap of at most k), then every frame at or below the k-th
void push_submap_indices(const std::vector<float>& dists, int k, const std::vector<int>& frames, std::vector<int>& out) {
  if (dists.empty()) return;
  std::priority_queue<float> pq;
  for (float d : dists) {
    if ((int)pq.size() >= k && pq.top() > d) {
      pq.push(d);
      pq.pop();
    } else if ((int)pq.size() < k) {
      pq.push(d);
    }
  }
  const float kth = pq.top();
  for (size_t i = 0; i < dists.size(); ++i)
    if (dists[i] <= kth) out.push_back(frames[i]);
}

}  // namespace

// ---------------------------------------------------------------------------
struct Keyframe {
  float pose[3];
  Quatf q;
  int n = 0;
  DevBuf pts;   // float4, world frame, original order (after the submap voxel filter)
  DevBuf cov;   // sym6 doubles, original order
};

struct ddlo_odom {
  int device = 0;
  ddlo_odom_params p{};
  gicp_ctx* s2s = nullptr;
  gicp_ctx* s2m = nullptr;
  hipStream_t s = nullptr;
  // scratch (device)
  DevBuf up, a, b, keep, pos, vscratch, cubtmp, medtmp, rng, rng_sorted, cat_pts, cat_cov;
  // ddlo_odom_set_voxel_order: the summation order of the scan and keyframe voxel
  // filters, and the scratch only the PCL order needs
  int voxel_order = DDLO_VOXEL_ORDER_INPUT;
  DevBuf voscratch;
  // ddlo_odom_set_downsampling: the row/column filter's registration pass in front of preprocess()
  int ds_use = 0, ds_row = 1, ds_col = 1, ds_rows = 1, ds_cols = 1;
  // ddlo_odom_set_intensity: the channel in the fourth lane of up -> a -> the keyframes, and the
  // preprocessed scan's intensities (original order) kept from preprocess() until make_keyframe
  int inten_use = 0;
  size_t inten_off = 0;
  DevBuf scan_w;
  // ddlo_odom_set_deskew (ddlo_deskew.h): the setting; the caller's twist for the next uploaded scan;
  // what the last scan got (source 0 none, 1 predicted, 2 the caller's); the last two poses T_ of
  // FIRST / TRACKED frames, [1] the newer, for the constant-velocity prediction
  ddlo_deskew_params dk{0, DDLO_TIME_F32_S, 12, 0.0, 0.1};
  bool dk_pending = false;
  double dk_pend_w[3] = {0, 0, 0}, dk_pend_t[3] = {0, 0, 0};
  int dk_source = 0;
  double dk_w[3] = {0, 0, 0}, dk_t[3] = {0, 0, 0};
  int dk_poses = 0;
  float dk_T[2][16];
  // pinned host memory: [0] the median range of the current scan, [4..19] the
  // voxel / crop count read-back (int)
  PinBuf median_pin;
  int* count_pin = nullptr;     // (inside median_pin)
  // the median range runs on the S2M stream (it is read after the S2S align),
  // beside the scan's index build: med_in = the voxel output is ready, med_done
  hipEvent_t med_in = nullptr, med_done = nullptr;
  // DDLO_ODOM_TIMING=1: host wall time per phase, printed at destroy (development)
  bool timing = false;
  double t_phase[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // [8] device drain before a frame, [9] H2D call
  long frames = 0;
  // state
  bool initialized = false;   // ddlo_initialized_
  bool have_target = false;
  float T[16], T_s2s[16], T_s2s_prev[16];
  float pose[3] = {0.f, 0.f, 0.f};
  Quatf rotq;
  std::vector<std::unique_ptr<Keyframe>> keyframes;
  std::vector<int> submap_prev, keyframe_convex, keyframe_concave;
  // the hulls are functions of the keyframe positions (append-only, never
  // moved) and, for the concave one, alpha: recomputed only when a keyframe
  // was added or alpha changed (the reference reruns qhull every scan; the
  // 3-D Delaunay of the concave hull costs ~0.1-0.6 ms of host time)
  int convex_nk = -1, concave_nk = -1;
  double concave_alpha = -1.0;
  bool have_median = false;
  float median_prev = 0.f;
  double thresh_dist = 1.0;
  int64_t submap_points = 0;
  // process_dynamic: the residual image, the frame's objects and the segments to cut out
  PinBuf resid_pin;
  std::vector<ddlo_seg_object> dyn_objs;
  std::vector<uint8_t> dyn_flags;
  std::vector<int32_t> dyn_remove;
  // process_tracked: time_prev_ (detection.cpp:62,824-825: it starts at 0 and advances only
  // on the frames that run the segmentation), and the frame's scratch
  double time_prev = 0.0;
  std::vector<int32_t> trk_ids, trk_set, trk_seg, trk_dead, trk_live, trk_status;
  std::vector<ddlo_map_box> trk_boxes;
};

// the dynamic-object step's arguments (ddlo_odom_process_dynamic)
struct DynStep {
  ddlo_seg* seg;
  ddlo_dynamic_params dp;
  ddlo_nonstatic_fn decide;
  void* user;
  ddlo_seg_result* seg_res;
  // ddlo_odom_process_tracked: the tracker decides, and the lists of its
  // non-static tracks (stale ones included) are what the keyframe loses
  ddlo_track* track = nullptr;
  ddlo_map* map = nullptr;
  double stamp = 0.0;
  ddlo_track_result* track_res = nullptr;
  // ddlo_odom_process_*_cloud: the scan is unorganized and reaches the image
  // through this projection (resolved and checked by the entry)
  bool cloud = false;
  ddlo_seg_projection proj{};
  ddlo_seg_projection_result* proj_res = nullptr;
};

namespace {

gicp_status ensure_tmp(ddlo_odom* o, int n) {
  const size_t t = std::max(crop_box_tmp_bytes(n), voxel_tmp_bytes(n));
  HIP_TRY(o->cubtmp.ensure(t));
  HIP_TRY(o->medtmp.ensure(median_tmp_bytes(n)));
  return GICP_OK;
}

// crop box + voxel filter of the float4 points in o->a (n) -> o->a; returns count.
// *finite_out (optional): the output is known finite, i.e. a crop pass ran (it
// drops non-finite points) or a voxel pass produced centroids (or nothing is
// left).  Not so when neither filter is on, or when the voxel grid overflowed
// with no crop box: the input is then passed on as it came, NaN points included.
gicp_status preprocess(ddlo_odom* o, int n, bool crop, double crop_size, bool vox, double leaf, int* nout,
                       bool* finite_out = nullptr) {
  if (finite_out) *finite_out = false;
  HIP_TRY(o->b.ensure(sizeof(float4) * (size_t)std::max(n, 1)));
  HIP_TRY(o->keep.ensure(sizeof(int) * (size_t)std::max(n, 1)));
  HIP_TRY(o->pos.ensure(sizeof(int) * (size_t)std::max(n, 1)));
  HIP_TRY(o->vscratch.ensure(sizeof(int) * voxel_scratch_ints(std::max(n, 1))));
  gicp_status st = ensure_tmp(o, std::max(n, 1));
  if (st) return st;
  const int order = o->voxel_order;
  if (vox && order != DDLO_VOXEL_ORDER_INPUT)
    HIP_TRY(o->voscratch.ensure(sizeof(int) * voxel_order_scratch_ints(std::max(n, 1))));
  int m = n;
  if (crop && vox && m > 0) {
    // one pass: the voxel filter over the points the crop box keeps (their
    // bbox, their input order), one count read-back instead of two
    int c = 0;
    if (voxel_grid(o->s, o->a.as<float4>(), m, (float)leaf, o->b.as<float4>(), o->vscratch.as<int>(), o->cubtmp.p,
                   o->cubtmp.bytes, &c, (float)crop_size, o->count_pin, CropCentre(), order, o->voscratch.as<int>(),
                   o->inten_use != 0))
      return fail(GICP_EHIP, "voxel filter scratch too small");
    if (c >= 0) {
      *nout = c;
      std::swap(o->a.p, o->b.p);
      std::swap(o->a.bytes, o->b.bytes);
      HIP_TRY(hipGetLastError());
      if (finite_out) *finite_out = true;
      return GICP_OK;
    }
    // grid overflow: the reference keeps the cropped cloud unchanged -> crop alone below
    vox = false;
  }
  bool finite = m <= 0;
  if (crop && m > 0) {
    finite = true;
    if (crop_box(o->s, o->a.as<float4>(), m, (float)crop_size, o->b.as<float4>(), o->keep.as<int>(), o->pos.as<int>(),
                 o->cubtmp.p, o->cubtmp.bytes, &m, o->count_pin))
      return fail(GICP_EHIP, "crop box scratch too small");
    std::swap(o->a.p, o->b.p);
    std::swap(o->a.bytes, o->b.bytes);
  }
  if (vox && m > 0) {
    int c = 0;
    if (voxel_grid(o->s, o->a.as<float4>(), m, (float)leaf, o->b.as<float4>(), o->vscratch.as<int>(), o->cubtmp.p,
                   o->cubtmp.bytes, &c, 0.f, o->count_pin, CropCentre(), order, o->voscratch.as<int>(),
                   o->inten_use != 0))
      return fail(GICP_EHIP, "voxel filter scratch too small");
    if (c >= 0) {  // -1: grid overflow, the reference keeps the cloud unchanged
      finite = true;
      m = c;
      std::swap(o->a.p, o->b.p);
      std::swap(o->a.bytes, o->b.bytes);
    }
  }
  HIP_TRY(hipGetLastError());
  *nout = m;
  if (finite_out) *finite_out = finite;
  return GICP_OK;
}

// device cloud from float4 points; `finite`: the points are known finite
// (preprocess() says so for a scan; keyframes, the submap), no read-back of the check
// with_cov: covariances follow (the scan, a keyframe), so nanoflann's tree
// for their tie order starts with the index build (not for the submap,
// whose covariances are the keyframes')
gicp_status cloud_from(ddlo_odom* o, gicp_ctx* c, const float4* pts, int n, std::shared_ptr<CloudData>* out,
                       bool finite, bool with_cov) {
  (void)o;
  return build_cloud(c, reinterpret_cast<const float*>(pts), (size_t)n, sizeof(float4), out, true, !finite, with_cov);
}

// keyframe from the n world-frame points in o->a: submap voxel filter, k-NN
// covariances with the S2S parameters (odom.cc:1133-1149)
gicp_status make_keyframe_from_a(ddlo_odom* o, int n) {
  auto kf = std::make_unique<Keyframe>();
  kf->pose[0] = o->pose[0];
  kf->pose[1] = o->pose[1];
  kf->pose[2] = o->pose[2];
  kf->q = o->rotq;
  int m = n;
  gicp_status st = preprocess(o, n, false, 0.0, o->p.vf_submap_use != 0, o->p.vf_submap_res, &m);
  if (st) return st;
  if (m < 1) return fail(GICP_ETOOFEW, "keyframe without points");
  kf->n = m;
  HIP_TRY(kf->pts.ensure(sizeof(float4) * (size_t)m));
  HIP_TRY(hipMemcpyAsync(kf->pts.p, o->a.p, sizeof(float4) * (size_t)m, hipMemcpyDeviceToDevice, o->s));
  // finite whatever preprocess() did (a grid overflow passes the input on):
  // the input is a scan cloud that passed cloud_from's check, transformed by
  // the pose, or seg_static_cloud_dev's output, which drops non-finite points
  // in its crop / voxel pass
  Side side;
  st = cloud_from(o, o->s2s, kf->pts.as<float4>(), m, &side.cloud, true, true);
  if (st) return st;
  // s2s->params: the S2S k (gicp_s2s_.calculateSourceCovariances); a
  // keyframe smaller than k uses all of its points (the reference reads
  // uninitialised neighbour slots there)
  st = compute_cov(o->s2s, side, std::min(o->p.s2s.k_correspondences, m));
  if (st) return st;
  HIP_TRY(kf->cov.ensure(sizeof(double) * 6 * (size_t)m));
  launch_gather_cov6(o->s, side.cov->cov6.as<double>(), side.cloud->perm.as<int>(), m, kf->cov.as<double>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(o->s));
  st = check_ties(o->s2s);   // the keyframe's (and the first scan's) covariance tie resolution
  if (st) return st;
  o->keyframes.push_back(std::move(kf));
  return GICP_OK;
}

// keyframe = world-frame copy of the (preprocessed) scan cloud (odom.cc:1129-1131)
gicp_status make_keyframe(ddlo_odom* o, const std::shared_ptr<CloudData>& scan) {
  const int n = scan->n;
  HIP_TRY(o->a.ensure(sizeof(float4) * (size_t)n));
  // (the registration contexts never see intensity: the sorted copy's w is a point index)
  launch_transform4(o->s, scan->pts.as<float4>(), scan->perm.as<int>(), n, o->T, o->a.as<float4>(),
                    o->inten_use ? o->scan_w.as<float>() : nullptr);
  return make_keyframe_from_a(o, n);
}

// keyframe = the segmented scan without its non-static objects
// (applySegmentation, odom.cc:887-918: segmentation_scan_t_ is what
// updateKeyframes stores), cropped around pose_ and voxel-filtered
gicp_status make_keyframe_static(ddlo_odom* o, const DynStep& d) {
  const float4* pts = nullptr;
  int n = 0;
  const double crop = o->p.crop_use ? o->p.crop_size : 0.0, leaf = o->p.vf_scan_use ? o->p.vf_scan_res : 0.0;
  gicp_status st = d.track ? seg_static_cloud_tracks_dev(d.seg, o->dyn_remove.data(), o->dyn_remove.size(), o->pose, crop,
                                                         leaf, &pts, &n, nullptr)
                           : seg_static_cloud_dev(d.seg, o->dyn_remove.data(), o->dyn_remove.size(), o->pose, crop, leaf,
                                                  &pts, &n);
  if (st) return st;
  if (n < 1) return fail(GICP_ETOOFEW, "keyframe without points");
  // (o->a is free: metrics() has waited for the median kernel, its last reader)
  HIP_TRY(o->a.ensure(sizeof(float4) * (size_t)n));
  HIP_TRY(hipMemcpyAsync(o->a.p, pts, sizeof(float4) * (size_t)n, hipMemcpyDeviceToDevice, o->s));
  return make_keyframe_from_a(o, n);
}

// trackDetections (detection.cpp:820-832) and what applySegmentation takes
// from the tracker (odom.cc:867-892), after the frame's objects: dt = stamp -
// time_prev_, TrackingModule::update, the pixel lists of the tracks this
// frame's detections updated or created replaced by their segments' and the
// erased tracks' released (ddlo_seg_tracks_sync), then dyn_remove = the ids
// of every UNDEFINED or DYNAMIC track: their lists, the stale ones of
// coasting tracks included, are what the keyframe loses.  With a map, the
// box histories of the tracks that turned dynamic are cleared from it.
// The tracker and time_prev_ advance first, as in the reference; an error in
// a later step (the sync, the map, the keyframe) leaves the tracker one frame
// ahead of the lists, and as every error of this driver it leaves the driver
// unusable (ddlo_odom.h): destroy the three handles together.  The collected
// boxes are taken from the tracker only once the sync has succeeded.
gicp_status tracked_step(ddlo_odom* o, const DynStep& d) {
  const size_t k = o->dyn_objs.size();
  const double dt = d.stamp - o->time_prev;
  o->time_prev = d.stamp;
  o->trk_ids.assign(k + 1, -1);
  ddlo_track_result tr{};
  gicp_status st = ddlo_track_update(d.track, dt, o->dyn_objs.data(), k, o->trk_ids.data(), &tr);
  if (st) return st;
  track_live(d.track, o->trk_live, o->trk_status);
  const std::vector<int>& erased = track_erased(d.track);
  // a track created and erased within this update (max_no_hits 0) never held a list
  o->trk_set.clear();
  o->trk_seg.clear();
  for (size_t i = 0; i < k; ++i)
    if (std::find(o->trk_live.begin(), o->trk_live.end(), o->trk_ids[i]) != o->trk_live.end()) {
      o->trk_set.push_back(o->trk_ids[i]);
      o->trk_seg.push_back(o->dyn_objs[i].id);
    }
  o->trk_dead.clear();
  for (int id : erased)
    if (std::find(o->trk_ids.begin(), o->trk_ids.begin() + (long)k, id) == o->trk_ids.begin() + (long)k)
      o->trk_dead.push_back(id);
  st = ddlo_seg_tracks_sync(d.seg, o->trk_set.data(), o->trk_seg.data(), o->trk_set.size(), o->trk_dead.data(),
                            o->trk_dead.size());
  if (st) return st;
  o->dyn_remove.clear();
  for (size_t i = 0; i < o->trk_live.size(); ++i)
    if (o->trk_status[i] != DDLO_TRACK_STATIC) o->dyn_remove.push_back(o->trk_live[i]);
  for (int32_t id : o->dyn_remove) {
    size_t len = 0;
    st = ddlo_seg_track_indices(d.seg, id, nullptr, 0, &len);
    if (st) return st;
    tr.indices_dropped += (int64_t)len;
  }
  size_t nb = 0;
  st = ddlo_track_take_cleared_boxes(d.track, nullptr, 0, &nb);
  if (st) return st;
  o->trk_boxes.resize(nb);
  if (nb) {
    st = ddlo_track_take_cleared_boxes(d.track, o->trk_boxes.data(), nb, &nb);
    if (st) return st;
    if (d.map) {
      st = ddlo_map_clear_boxes(d.map, o->trk_boxes.data(), nb, nullptr);
      if (st) return st;
    }
  }
  if (d.track_res) *d.track_res = tr;
  return GICP_OK;
}

// OdomNode::applySegmentation up to the tracker's verdict (odom.cc:853-870),
// on a tracked frame after propagateS2M: o->up still holds the frame's scan
// (npts points, stride bytes apart): organized, rows x cols of them, or
// (d.cloud) unorganized, projected into the image by the claim and the fill
gicp_status dynamic_step(ddlo_odom* o, const DynStep& d, int npts, size_t stride) {
  ddlo_seg_params sp;
  gicp_status st = seg_get_params(d.seg, &sp);
  if (st) return st;
  const int npix = sp.rows * sp.cols;
  if (d.cloud) {
    ddlo_seg_projection_result pr{};
    st = seg_project_dev(d.seg, o->s, o->up.as<unsigned char>(), stride, npts, o->T, d.proj, &pr,
                         o->inten_use ? o->inten_off : 0);
    if (st) return st;
    if (d.proj_res) *d.proj_res = pr;
  } else {
    float4* buf = nullptr;
    int n = 0;
    st = seg_stage_input(d.seg, &buf, &n);
    if (st) return st;
    if (n != npts) return fail(GICP_EINVAL, "scan size != the segmentation's rows x cols");
    launch_transform_raw(o->s, o->up.as<unsigned char>(), stride, npts, o->T, buf, o->inten_use ? o->inten_off : 0);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(o->s));
  }
  HIP_TRY(o->resid_pin.ensure(sizeof(float) * (size_t)npix));
  float* const resid = o->resid_pin.as<float>();
  st = gicp_residual_image(o->s2m, d.dp.theta_min, d.dp.theta_max, sp.cols, sp.rows, resid, nullptr);
  if (st) return st;
  ddlo_seg_result sr{};
  st = seg_process_staged(d.seg, o->T, resid, &sr);
  if (st) return st;
  if (d.cloud) {
    st = seg_project_commit(d.seg);
    if (st) return st;
  }
  if (d.seg_res) *d.seg_res = sr;
  st = seg_objects_vec(d.seg, d.dp.max_dim_ratio, o->dyn_objs);
  if (st) return st;
  const size_t k = o->dyn_objs.size();
  if (d.track) return tracked_step(o, d);
  o->dyn_flags.assign(k + 1, 0);
  if (d.decide) {
    if (d.decide(d.user, o->dyn_objs.data(), k, o->dyn_flags.data()) != 0)
      return fail(GICP_ESTATE, "the non-static callback aborted the scan");
  } else {
    std::fill(o->dyn_flags.begin(), o->dyn_flags.end(), (uint8_t)1);
  }
  o->dyn_remove.clear();
  for (size_t i = 0; i < k; ++i)
    if (o->dyn_flags[i]) o->dyn_remove.push_back(o->dyn_objs[i].id);
  return GICP_OK;
}

// OdomNode::getSubmapKeyframes (odom.cc:1215-1315); returns whether it changed
gicp_status submap_keyframes(ddlo_odom* o, bool* changed) {
  const int nk = (int)o->keyframes.size();
  std::vector<int> cur;
  std::vector<float> ds;
  std::vector<int> nn;
  const float cx = o->T_s2s[3], cy = o->T_s2s[7], cz = o->T_s2s[11];
  for (int i = 0; i < nk; ++i) {
    const float* k = o->keyframes[i]->pose;
    ds.push_back((float)std::sqrt(std::pow(cx - k[0], 2) + std::pow(cy - k[1], 2) + std::pow(cz - k[2], 2)));
    nn.push_back(i);
  }
  push_submap_indices(ds, o->p.submap_knn, nn, cur);
  std::vector<float> kpos(3 * (size_t)nk);
  for (int i = 0; i < nk; ++i)
    for (int a = 0; a < 3; ++a) kpos[3 * i + a] = o->keyframes[i]->pose[a];
  if (nk >= 4 && nk != o->convex_nk) {   // computeConvexHull: >= 4 keyframes
    o->keyframe_convex = convex_hull(kpos.data(), nk);
    o->convex_nk = nk;
  }
  std::vector<float> cds;
  for (int c : o->keyframe_convex) cds.push_back(ds[c]);
  push_submap_indices(cds, o->p.submap_kcv, o->keyframe_convex, cur);
  if (nk >= 5 && (nk != o->concave_nk || o->thresh_dist != o->concave_alpha)) {   // >= 5 keyframes
    o->keyframe_concave = concave_hull(kpos.data(), nk, o->thresh_dist);
    o->concave_nk = nk;
    o->concave_alpha = o->thresh_dist;
  }
  std::vector<float> kds;
  for (int c : o->keyframe_concave) kds.push_back(ds[c]);
  push_submap_indices(kds, o->p.submap_kcc, o->keyframe_concave, cur);
  std::sort(cur.begin(), cur.end());
  cur.erase(std::unique(cur.begin(), cur.end()), cur.end());
  *changed = cur != o->submap_prev;
  if (!*changed) return GICP_OK;
  // submap cloud + normals: the selected keyframes concatenated in index
  // order, all on the device
  int64_t total = 0;
  for (int k : cur) total += o->keyframes[k]->n;
  if (total > INT32_MAX / 2) return fail(GICP_EINVAL, "submap too large");
  HIP_TRY(o->cat_pts.ensure(sizeof(float4) * (size_t)total));
  HIP_TRY(o->cat_cov.ensure(sizeof(double) * 6 * (size_t)total));
  // everything of the submap build runs on the S2M context's stream: the
  // concatenation, its index (build_cloud) and the covariance import
  hipStream_t sm = o->s2m->stream;
  int64_t off = 0;
  for (int k : cur) {
    const Keyframe& kf = *o->keyframes[k];
    HIP_TRY(hipMemcpyAsync(o->cat_pts.as<float4>() + off, kf.pts.p, sizeof(float4) * kf.n, hipMemcpyDeviceToDevice, sm));
    HIP_TRY(hipMemcpyAsync(o->cat_cov.as<double>() + 6 * off, kf.cov.p, sizeof(double) * 6 * kf.n,
                           hipMemcpyDeviceToDevice, sm));
    off += kf.n;
  }
  Side tgt;
  gicp_status st = cloud_from(o, o->s2m, o->cat_pts.as<float4>(), (int)total, &tgt.cloud, true, false);
  if (st) return st;
  auto cv = std::make_shared<CovData>();
  cv->n = (int)total;
  HIP_TRY(cv->cov6.ensure(sizeof(double) * 6 * (size_t)total));
  launch_cov_import(sm, o->cat_cov.as<double>(), GICP_COV_SYM6, (int)total, tgt.cloud->inv_perm.as<int>(),
                    cv->cov6.as<double>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(sm));
  tgt.cov = cv;
  o->s2m->tgt = tgt;        // setInputTarget + setTargetCovariances (odom.cc:780-783)
  invalidate_align(o->s2m);
  o->submap_prev = cur;
  o->submap_points = total;
  return GICP_OK;
}

void copy_pose(const float* T, float* out) { std::memcpy(out, T, sizeof(float) * 16); }

// ddlo_intensity.h's rules for the place of the intensity in a record
bool intensity_offset_ok(size_t off, size_t stride) { return off % 4 == 0 && off >= 12 && off + 4 <= stride; }
// the bytes of n records that are read: x, y, z of the last one, its intensity if that is on, and
// its time (tend = the byte after the time field) if deskew is on
size_t raw_bytes(size_t n, size_t stride, size_t ioff, size_t tend = 0) {
  return (n - 1) * stride + std::max(std::max<size_t>(12, ioff ? ioff + 4 : 0), tend);
}

// ddlo_deskew.h: the twist of the scan just uploaded into o->up (the caller's, for this scan only, or
// the prediction from the last two poses) and the in-place pass, on o->s behind the copy
void deskew_upload(ddlo_odom* o, int n, size_t stride) {
  if (o->dk_pending) {
    o->dk_pending = false;
    std::memcpy(o->dk_w, o->dk_pend_w, sizeof(o->dk_w));
    std::memcpy(o->dk_t, o->dk_pend_t, sizeof(o->dk_t));
    o->dk_source = 2;
  } else if (o->dk_poses >= 2) {
    deskew_between(o->dk_T[0], o->dk_T[1], o->dk_w, o->dk_t);
    o->dk_source = 1;
  }
  DeskewTwist w;
  if (o->dk_source && deskew_twist(o->dk_w, o->dk_t, o->dk.ref_time, o->dk.period, &w))
    launch_deskew(o->s, o->up.as<unsigned char>(), stride, n, o->dk.time_type, o->dk.time_offset_bytes, w);
  else
    o->dk_source = 0;
}

// a pose T_ the driver produced (FIRST: the identity; TRACKED) joins the prediction's history
void deskew_push_pose(ddlo_odom* o) {
  std::memcpy(o->dk_T[0], o->dk_T[1], sizeof(float) * 16);
  std::memcpy(o->dk_T[1], o->T, sizeof(float) * 16);
  o->dk_poses = std::min(o->dk_poses + 1, 2);
}

// the n uploaded points of o->up into o->a as float4; returns how many.  With
// the row/column filter on: only the pixels of S below n, ascending, unless
// |S| > n, when ExtractIndices reports an error and passes the scan on as it is
int pack_scan(ddlo_odom* o, int n, size_t stride) {
  if (o->ds_use && rowcol_size(o->ds_rows, o->ds_cols, o->ds_row, o->ds_col) <= (long long)n)
    return launch_pack4_rowcol(o->s, o->up.as<unsigned char>(), stride, n, o->ds_rows, o->ds_cols, o->ds_row, o->ds_col,
                               o->a.as<float4>(), o->inten_use ? o->inten_off : 0);
  launch_pack4(o->s, o->up.as<unsigned char>(), stride, n, o->a.as<float4>(), o->inten_use ? o->inten_off : 0);
  return n;
}

// what ddlo_odom_set_downsampling asks of a scan and of the segmentation
// handle, checked before anything of the scan or the driver's state is touched
gicp_status downsampling_check(const ddlo_odom* o, size_t n, const DynStep* dyn) {
  int use = 0, row = 1, col = 1;
  if (dyn) {
    gicp_status st = ddlo_seg_get_downsampling(dyn->seg, &use, &row, &col);
    if (st) return st;
    if ((use != 0) != (o->ds_use != 0))
      return fail(GICP_EINVAL, "downsampling is on for one of the driver and the segmentation only");
  }
  if (!o->ds_use) return GICP_OK;
  if (dyn && dyn->cloud) return fail(GICP_EINVAL, "downsampling needs an organized scan: not with the _cloud entries");
  if (n != (size_t)o->ds_rows * (size_t)o->ds_cols) return fail(GICP_EINVAL, "downsampling: scan size != rows x cols");
  if (dyn) {
    ddlo_seg_params sp;
    gicp_status st = seg_get_params(dyn->seg, &sp);
    if (st) return st;
    if (sp.rows != o->ds_rows || sp.cols != o->ds_cols)
      return fail(GICP_EINVAL, "downsampling: the segmentation's rows x cols differ from the driver's");
    if (row != o->ds_row || col != o->ds_col)
      return fail(GICP_EINVAL, "downsampling: the segmentation's steps differ from the driver's");
  }
  return GICP_OK;
}

}  // namespace

extern "C" {

gicp_status ddlo_odom_default_params(ddlo_odom_params* p) {
  if (!p) return fail(GICP_EINVAL, "null params");
  std::memset(p, 0, sizeof(*p));
  gicp_default_params(&p->s2s);
  gicp_default_params(&p->s2m);
  // cfg/ddlo.yaml:185-204
  p->s2s.k_correspondences = 10;
  p->s2s.max_correspondence_distance = 1.0;
  p->s2s.max_iterations = 32;
  p->s2s.transformation_epsilon = 0.01;
  p->s2m.k_correspondences = 20;
  p->s2m.max_correspondence_distance = 2.0;
  p->s2m.max_iterations = 32;
  p->s2m.transformation_epsilon = 0.01;
  p->min_num_points = 10;
  p->keyframe_thresh_dist = 1.0;
  p->keyframe_thresh_rot = 0.1;
  p->submap_knn = p->submap_kcv = p->submap_kcc = 10;
  p->adaptive = 1;
  p->crop_use = 1;
  p->crop_size = 1.0;
  p->vf_scan_use = 1;
  p->vf_scan_res = 0.1;
  p->vf_submap_use = 1;
  p->vf_submap_res = 0.1;
  p->skip_first_scan = 1;
  p->s2m_target_grid = GICP_GRID_OFF;
  return GICP_OK;
}

gicp_status ddlo_odom_create(int device, const ddlo_odom_params* p, ddlo_odom** out) {
  if (!out) return fail(GICP_EINVAL, "null out");
  *out = nullptr;
  auto o = std::make_unique<ddlo_odom>();
  if (p) {
    o->p = *p;
  } else {
    ddlo_odom_default_params(&o->p);
  }
  if (o->p.submap_knn < 1 || o->p.submap_kcv < 1 || o->p.submap_kcc < 1) return fail(GICP_EINVAL, "submap k must be >= 1");
  if ((o->p.vf_scan_use && !(o->p.vf_scan_res > 0)) || (o->p.vf_submap_use && !(o->p.vf_submap_res > 0)))
    return fail(GICP_EINVAL, "voxel resolution must be positive");
  o->device = device;
  gicp_status st = gicp_ctx_create(device, &o->s2s);
  if (!st) st = gicp_ctx_create(device, &o->s2m);
  if (!st) st = gicp_set_params(o->s2s, &o->p.s2s);
  if (!st) st = gicp_set_params(o->s2m, &o->p.s2m);
  if (!st) st = gicp_set_target_grid(o->s2m, o->p.s2m_target_grid);
  if (!st) st = gicp_set_target_grid(o->s2s, GICP_GRID_OFF);   // S2S targets live one scan
  if (st) {
    if (o->s2s) gicp_ctx_destroy(o->s2s);
    if (o->s2m) gicp_ctx_destroy(o->s2m);
    return st;
  }
  o->s = o->s2s->stream;  // one stream: the driver's work is one dependent chain
  o->timing = dev_getenv("DDLO_ODOM_TIMING") != nullptr;
  if (o->median_pin.reset(sizeof(float) * 20) != hipSuccess ||
      hipEventCreateWithFlags(&o->med_in, hipEventDisableTiming) != hipSuccess ||
      hipEventCreateWithFlags(&o->med_done, hipEventDisableTiming) != hipSuccess) {
    if (o->med_in) (void)hipEventDestroy(o->med_in);
    gicp_ctx_destroy(o->s2s);
    gicp_ctx_destroy(o->s2m);
    return fail(GICP_EHIP, "pinned allocation failed");
  }
  *o->median_pin.as<float>() = 0.f;
  o->count_pin = reinterpret_cast<int*>(o->median_pin.as<float>() + 4);
  mat4_identity(o->T);
  mat4_identity(o->T_s2s);
  mat4_identity(o->T_s2s_prev);
  o->thresh_dist = o->p.keyframe_thresh_dist;
  *out = o.release();
  return GICP_OK;
}

gicp_status ddlo_odom_destroy(ddlo_odom* o) {
  if (!o) return GICP_OK;
  (void)hipSetDevice(o->device);
  (void)hipStreamSynchronize(o->s2m->stream);
  (void)hipStreamSynchronize(o->s);
  if (o->timing && o->frames > 0) {
    static const char* names[10] = {"upload", "preprocess", "cloud", "s2s_align", "submap", "s2m_align", "keyframe",
                                    "total", "drain_before", "h2d_call"};
    std::fprintf(stderr, "[odom timing] %ld frames, us/frame:", o->frames);
    for (int k = 0; k < 10; ++k) std::fprintf(stderr, " %s %.1f", names[k], 1e6 * o->t_phase[k] / o->frames);
    std::fprintf(stderr, "\n");
  }
  o->keyframes.clear();
  if (o->med_in) (void)hipEventDestroy(o->med_in);
  if (o->med_done) (void)hipEventDestroy(o->med_done);
  gicp_ctx_destroy(o->s2m);
  gicp_ctx_destroy(o->s2s);
  delete o;
  return GICP_OK;
}

// OdomNode::icpCB; dyn: the dynamic-object step of ddlo_odom_process_dynamic (else nullptr)
static gicp_status process_scan(ddlo_odom* o, const float* xyz, size_t n, size_t stride, ddlo_odom_result* res,
                                const DynStep* dyn) {
  if (!o || !res || (!xyz && n) || stride < 12 || stride % 4) return fail(GICP_EINVAL, "invalid argument");
  if (n > (size_t)INT32_MAX / 2) return fail(GICP_EINVAL, "scan too large");
  if (o->inten_use && !intensity_offset_ok(o->inten_off, stride))
    return fail(GICP_EINVAL, "intensity offset: a multiple of 4, >= 12 and offset + 4 <= stride");
  if (o->dk.use)
    if (const char* e = deskew_field_error(o->dk.time_type, o->dk.time_offset_bytes, stride, o->inten_use != 0, o->inten_off))
      return fail(GICP_EINVAL, e);
  if (dyn) {   // the keyframes come from the segmentation's static cloud: both carry the channel, or neither
    int seg_use = 0;
    if (gicp_status e = ddlo_seg_get_intensity(dyn->seg, &seg_use, nullptr)) return e;
    if ((seg_use != 0) != (o->inten_use != 0))
      return fail(GICP_EINVAL, "intensity is on for one of the driver and the segmentation only");
  }
  gicp_status st = downsampling_check(o, n, dyn);
  if (st) return st;
  st = set_device(o->s2s);
  if (st) return st;
  begin_ties(o->s2s);
  begin_ties(o->s2m);
  o->dk_source = 0;   // (an INIT or SKIPPED frame deskews nothing and keeps a pending twist)
  std::memset(res, 0, sizeof(*res));
  copy_pose(o->T, res->T);
  copy_pose(o->T_s2s, res->T_s2s);
  mat4_identity(res->T_s2s_local);
  res->num_keyframes = (int)o->keyframes.size();
  // icpCB: too few points -> return (odom.cc:635-639)
  if ((int64_t)n < o->p.min_num_points) {
    res->status = DDLO_ODOM_SKIPPED;
    return GICP_OK;
  }
  // DLO initialisation consumes the first valid scan (odom.cc:641-646;
  // gravity alignment is out of scope, so it only sets ddlo_initialized_)
  if (!o->initialized) {
    o->initialized = true;
    if (o->p.skip_first_scan) {
      res->status = DDLO_ODOM_INIT;
      return GICP_OK;
    }
  }
  using clk = std::chrono::steady_clock;
  if (o->timing) {   // work of the previous frame still queued on any stream (aux included)
    const auto td = clk::now();
    (void)hipDeviceSynchronize();
    o->t_phase[8] += std::chrono::duration<double>(clk::now() - td).count();
  }
  auto t0 = clk::now(), tl = t0;
  auto mark = [&](int k) {
    if (!o->timing) return;
    (void)hipStreamSynchronize(o->s);
    (void)hipStreamSynchronize(o->s2m->stream);
    const auto t = clk::now();
    o->t_phase[k] += std::chrono::duration<double>(t - tl).count();
    tl = t;
  };
  // upload + preprocessPoints (odom.cc:442-478)
  const int N = (int)n;
  const size_t raw = raw_bytes(n, stride, o->inten_use ? o->inten_off : 0,
                               o->dk.use ? o->dk.time_offset_bytes + (o->dk.time_type == DDLO_TIME_F64_S ? 8 : 4) : 0);
  HIP_TRY(o->up.ensure(raw));
  HIP_TRY(hipMemcpyAsync(o->up.p, xyz, raw, hipMemcpyHostToDevice, o->s));
  // the whole scan, before the registration pack: every reader of o->up sees the deskewed frame
  if (o->dk.use) deskew_upload(o, N, stride);
  else o->dk_pending = false;
  if (o->timing) o->t_phase[9] += std::chrono::duration<double>(clk::now() - t0).count();
  HIP_TRY(o->a.ensure(sizeof(float4) * n));
  // the registration scan: every point, or only the row/column filter's pixels
  // (odom.cc:445-455); o->up keeps the whole scan for the segmentation
  const int NR = pack_scan(o, N, stride);
  mark(0);
  int m = NR;
  bool scan_finite = false;
  st = preprocess(o, NR, o->p.crop_use != 0, o->p.crop_size, o->p.vf_scan_use != 0, o->p.vf_scan_res, &m, &scan_finite);
  if (st) return st;
  res->scan_points = m;
  if (o->inten_use) {   // o->a is the keyframe's staging buffer later: the channel is set aside now
    HIP_TRY(o->scan_w.ensure(sizeof(float) * (size_t)std::max(m, 1)));
    launch_take_w(o->s, o->a.as<float4>(), m, o->scan_w.as<float>());
  }
  mark(1);
  // computeSpaciousness (odom.cc:981-1001): the median range is selected on
  // the device and copied to pinned memory, on the S2M context's stream (idle
  // until the submap build) beside the scan's index build and the S2S align;
  // metrics() waits for it (nothing before scan matching uses it).  The scan
  // (o->a) is not written again before that wait.
  HIP_TRY(o->rng.ensure(sizeof(float) * (size_t)std::max(m, 1)));
  HIP_TRY(o->rng_sorted.ensure(sizeof(float) * (size_t)std::max(m, 1)));
  {
    hipStream_t sm = o->s2m->stream;
    HIP_TRY(hipEventRecord(o->med_in, o->s));
    HIP_TRY(hipStreamWaitEvent(sm, o->med_in, 0));
    if (m > 0)
      median_range_async(sm, o->a.as<float4>(), m, o->rng.as<float>(), o->rng_sorted.as<float>(), o->medtmp.p,
                         o->medtmp.bytes, o->median_pin.as<float>());
    else
      *o->median_pin.as<float>() = 0.f;
    HIP_TRY(hipEventRecord(o->med_done, sm));
  }
  // computeMetrics + setAdaptiveParams (odom.cc:981-1001, 1156-1178), once
  // the median has arrived
  auto metrics = [&]() {
    (void)hipEventSynchronize(o->med_done);
    const float median_curr = *o->median_pin.as<float>();
    if (!o->have_median) {  // static float median_prev = median_curr (first call)
      o->median_prev = median_curr;
      o->have_median = true;
    }
    const float median_lpf = (float)(0.95 * o->median_prev + 0.05 * median_curr);
    o->median_prev = median_lpf;
    res->spaciousness = median_lpf;
    if (o->p.adaptive) {
      if (median_lpf > 20.0) o->thresh_dist = 10.0;
      else if (median_lpf > 10.0 && median_lpf <= 20.0) o->thresh_dist = 5.0;
      else if (median_lpf > 5.0 && median_lpf <= 10.0) o->thresh_dist = 1.0;
      else if (median_lpf <= 5.0) o->thresh_dist = 0.5;
    }
    res->keyframe_thresh_dist = o->thresh_dist;
  };
  if (m < std::max(o->p.s2s.k_correspondences, o->p.s2m.k_correspondences)) {
    HIP_TRY(hipStreamSynchronize(o->s));
    metrics();
    return fail(GICP_ETOOFEW, "preprocessed scan has fewer points than k_correspondences");
  }
  // the preprocessed scan as a device cloud (checked for non-finite points
  // unless the preprocessing is known to have dropped them)
  std::shared_ptr<CloudData> scan;
  st = cloud_from(o, o->s2s, o->a.as<float4>(), m, &scan, scan_finite, true);
  if (st) return st;
  mark(2);

  if (!o->have_target) {
    // initializeInputTarget (odom.cc:480-516)
    o->s2s->tgt = Side();
    o->s2s->tgt.cloud = scan;
    invalidate_align(o->s2s);
    st = compute_cov(o->s2s, o->s2s->tgt);   // calculateTargetCovariances
    if (st) return st;
    st = make_keyframe(o, scan);              // T_ = identity: the scan itself (waits for the stream)
    if (st) return st;
    metrics();
    o->have_target = true;
    deskew_push_pose(o);
    if (dyn && dyn->map) {   // MapNode::keyframeCB receives the first keyframe as every other
      st = ddlo_map_add_odom_keyframe(dyn->map, o, (int)o->keyframes.size() - 1, nullptr);
      if (st) return st;
    }
    res->status = DDLO_ODOM_FIRST;
    res->keyframe_added = 1;
    res->num_keyframes = (int)o->keyframes.size();
    return GICP_OK;
  }
  // setInputSources (odom.cc:518-532): one device cloud for both
  o->s2s->src = Side();
  o->s2s->src.cloud = scan;
  invalidate_align(o->s2s);
  o->s2m->src = Side();
  o->s2m->src.cloud = scan;
  invalidate_align(o->s2m);

  // scanMatching (odom.cc:745-851)
  float T_S2S[16];
  st = gicp_align(o->s2s, nullptr, T_S2S, &res->s2s);   // waits for the stream: the median has arrived
  if (st) return st;
  mark(3);
  metrics();
  copy_pose(T_S2S, res->T_s2s_local);
  mat4_mul(o->T_s2s_prev, T_S2S, o->T_s2s);   // propagateS2S
  copy_pose(o->T_s2s, o->T_s2s_prev);
  o->s2m->src.cov = o->s2s->src.cov;          // gicp_s2m_.source_covs_ = gicp_s2s_.source_covs_
  gicp_swap_source_target(o->s2s);            // the scan becomes the next S2S target
  bool changed = false;
  st = submap_keyframes(o, &changed);
  if (st) return st;
  mark(4);
  st = gicp_align(o->s2m, o->T_s2s, o->T, &res->s2m);
  if (st) return st;
  mark(5);
  copy_pose(o->T, o->T_s2s_prev);             // T_s2s_prev_ = T_
  o->pose[0] = o->T[3];                       // propagateS2M
  o->pose[1] = o->T[7];
  o->pose[2] = o->T[11];
  o->rotq = quat_from_R(o->T);
  deskew_push_pose(o);
  if (dyn) {
    st = dynamic_step(o, *dyn, N, stride);
    if (st) return st;
  }

  // updateKeyframes (odom.cc:1067-1154)
  {
    float closest_d = INFINITY;
    int closest = 0, idx = 0, num_nearby = 0;
    for (const auto& k : o->keyframes) {
      const float dd = (float)std::sqrt(std::pow(o->pose[0] - k->pose[0], 2) + std::pow(o->pose[1] - k->pose[1], 2) +
                                        std::pow(o->pose[2] - k->pose[2], 2));
      if (dd <= o->thresh_dist * 1.5) ++num_nearby;
      if (dd < closest_d) {
        closest_d = dd;
        closest = idx;
      }
      ++idx;
    }
    const Keyframe& ck = *o->keyframes[closest];
    const float dd = (float)std::sqrt(std::pow(o->pose[0] - ck.pose[0], 2) + std::pow(o->pose[1] - ck.pose[1], 2) +
                                      std::pow(o->pose[2] - ck.pose[2], 2));
    const Quatf dq = quat_mul(o->rotq, quat_inverse(ck.q));
    const float theta_rad = (float)(2. * std::atan2(std::sqrt(std::pow(dq.x, 2) + std::pow(dq.y, 2) + std::pow(dq.z, 2)), dq.w));
    const float theta_deg = (float)(theta_rad * (180.0 / M_PI));
    bool add = false;
    if (std::fabs(dd) > o->thresh_dist || std::fabs(theta_deg) > o->p.keyframe_thresh_rot) add = true;
    if (std::fabs(dd) <= o->thresh_dist) add = false;
    if (std::fabs(dd) <= o->thresh_dist && std::fabs(theta_deg) > o->p.keyframe_thresh_rot && num_nearby <= 1) add = true;
    if (add) {
      // registration_scan_t_ = T_ * scan (transformScans), or the segmented scan without its non-static objects
      st = dyn ? make_keyframe_static(o, *dyn) : make_keyframe(o, scan);
      if (st) return st;
      res->keyframe_added = 1;
      if (dyn && dyn->map) {   // MapNode::keyframeCB for the keyframe just published
        st = ddlo_map_add_odom_keyframe(dyn->map, o, (int)o->keyframes.size() - 1, nullptr);
        if (st) return st;
      }
    }
  }
  mark(6);
  if (o->timing) {
    o->t_phase[7] += std::chrono::duration<double>(clk::now() - t0).count();
    ++o->frames;
  }
  res->status = DDLO_ODOM_TRACKED;
  copy_pose(o->T, res->T);
  copy_pose(o->T_s2s, res->T_s2s);
  res->submap_changed = changed ? 1 : 0;
  res->num_keyframes = (int)o->keyframes.size();
  res->submap_keyframes = (int)o->submap_prev.size();
  res->submap_points = o->submap_points;
  return GICP_OK;
}

gicp_status ddlo_odom_process(ddlo_odom* o, const float* xyz, size_t n, size_t stride, ddlo_odom_result* res) {
  return process_scan(o, xyz, n, stride, res, nullptr);
}

gicp_status ddlo_dynamic_default_params(ddlo_dynamic_params* p) {
  if (!p) return fail(GICP_EINVAL, "null params");
  p->theta_min = -60 * M_PI / 180;   // odom.cc:804-805
  p->theta_max = 60 * M_PI / 180;
  p->max_dim_ratio = 10.0f;          // detection.cpp:106
  return GICP_OK;
}

gicp_status ddlo_odom_process_dynamic(ddlo_odom* o, ddlo_seg* seg, const float* xyz, size_t stride,
                                      const ddlo_dynamic_params* dp, ddlo_nonstatic_fn decide, void* user,
                                      ddlo_odom_result* res, ddlo_seg_result* seg_res) {
  if (!o || !seg || !xyz || !res) return fail(GICP_EINVAL, "null argument");
  if (seg_device(seg) != o->device) return fail(GICP_EINVAL, "the segmentation lives on another device");
  ddlo_seg_params sp;
  gicp_status st = seg_get_params(seg, &sp);
  if (st) return st;
  DynStep d{seg, {}, decide, user, seg_res};
  if (dp) d.dp = *dp;
  else ddlo_dynamic_default_params(&d.dp);
  if (!(d.dp.theta_max > d.dp.theta_min)) return fail(GICP_EINVAL, "theta_max must exceed theta_min");
  if (seg_res) std::memset(seg_res, 0, sizeof(*seg_res));
  return process_scan(o, xyz, (size_t)sp.rows * sp.cols, stride, res, &d);
}

gicp_status ddlo_odom_process_tracked(ddlo_odom* o, ddlo_seg* seg, ddlo_track* track, ddlo_map* map, const float* xyz,
                                      size_t stride, double stamp, const ddlo_dynamic_params* dp, ddlo_odom_result* res,
                                      ddlo_seg_result* seg_res, ddlo_track_result* track_res) {
  if (!o || !seg || !track || !xyz || !res) return fail(GICP_EINVAL, "null argument");
  if (seg_device(seg) != o->device) return fail(GICP_EINVAL, "the segmentation lives on another device");
  if (!std::isfinite(stamp)) return fail(GICP_EINVAL, "non-finite stamp");
  ddlo_seg_params sp;
  gicp_status st = seg_get_params(seg, &sp);
  if (st) return st;
  DynStep d{seg, {}, nullptr, nullptr, seg_res};
  d.track = track;
  d.map = map;
  d.stamp = stamp;
  d.track_res = track_res;
  if (dp) d.dp = *dp;
  else ddlo_dynamic_default_params(&d.dp);
  if (!(d.dp.theta_max > d.dp.theta_min)) return fail(GICP_EINVAL, "theta_max must exceed theta_min");
  if (seg_res) std::memset(seg_res, 0, sizeof(*seg_res));
  if (track_res) std::memset(track_res, 0, sizeof(*track_res));
  return process_scan(o, xyz, (size_t)sp.rows * sp.cols, stride, res, &d);
}

// the *_cloud entries' part of a DynStep: the projection resolved and checked before anything runs
static gicp_status cloud_step(DynStep* d, const ddlo_seg_projection* proj, ddlo_seg_projection_result* proj_res) {
  d->cloud = true;
  d->proj_res = proj_res;
  if (proj_res) std::memset(proj_res, 0, sizeof(*proj_res));
  return seg_projection_resolve(d->seg, proj, &d->proj);
}

gicp_status ddlo_odom_process_dynamic_cloud(ddlo_odom* o, ddlo_seg* seg, const float* xyz, size_t stride, size_t n,
                                            const ddlo_dynamic_params* dp, ddlo_nonstatic_fn decide, void* user,
                                            const ddlo_seg_projection* proj, ddlo_odom_result* res,
                                            ddlo_seg_result* seg_res, ddlo_seg_projection_result* proj_res) {
  if (!o || !seg || (!xyz && n) || !res) return fail(GICP_EINVAL, "null argument");
  if (seg_device(seg) != o->device) return fail(GICP_EINVAL, "the segmentation lives on another device");
  DynStep d{seg, {}, decide, user, seg_res};
  if (dp) d.dp = *dp;
  else ddlo_dynamic_default_params(&d.dp);
  if (!(d.dp.theta_max > d.dp.theta_min)) return fail(GICP_EINVAL, "theta_max must exceed theta_min");
  if (gicp_status st = cloud_step(&d, proj, proj_res)) return st;
  if (seg_res) std::memset(seg_res, 0, sizeof(*seg_res));
  return process_scan(o, xyz, n, stride, res, &d);
}

gicp_status ddlo_odom_process_tracked_cloud(ddlo_odom* o, ddlo_seg* seg, ddlo_track* track, ddlo_map* map,
                                            const float* xyz, size_t stride, size_t n, double stamp,
                                            const ddlo_dynamic_params* dp, const ddlo_seg_projection* proj,
                                            ddlo_odom_result* res, ddlo_seg_result* seg_res, ddlo_track_result* track_res,
                                            ddlo_seg_projection_result* proj_res) {
  if (!o || !seg || !track || (!xyz && n) || !res) return fail(GICP_EINVAL, "null argument");
  if (seg_device(seg) != o->device) return fail(GICP_EINVAL, "the segmentation lives on another device");
  if (!std::isfinite(stamp)) return fail(GICP_EINVAL, "non-finite stamp");
  DynStep d{seg, {}, nullptr, nullptr, seg_res};
  d.track = track;
  d.map = map;
  d.stamp = stamp;
  d.track_res = track_res;
  if (dp) d.dp = *dp;
  else ddlo_dynamic_default_params(&d.dp);
  if (!(d.dp.theta_max > d.dp.theta_min)) return fail(GICP_EINVAL, "theta_max must exceed theta_min");
  if (gicp_status st = cloud_step(&d, proj, proj_res)) return st;
  if (seg_res) std::memset(seg_res, 0, sizeof(*seg_res));
  if (track_res) std::memset(track_res, 0, sizeof(*track_res));
  return process_scan(o, xyz, n, stride, res, &d);
}

gicp_status ddlo_odom_classify(ddlo_seg* seg, const ddlo_track* track, ddlo_seg_class_counts* counts) {
  if (!seg || !track) return fail(GICP_EINVAL, "null argument");
  std::vector<int32_t> ids, status;
  track_live(track, ids, status);
  return ddlo_seg_classify(seg, ids.data(), status.data(), ids.size(), counts);
}

gicp_status ddlo_odom_keyframe_points(const ddlo_odom* o, int k, float* xyz, size_t cap, size_t* n) {
  if (!o || !n || (!xyz && cap) || k < 0 || k >= (int)o->keyframes.size()) return fail(GICP_EINVAL, "invalid argument");
  const Keyframe& kf = *o->keyframes[k];
  *n = (size_t)kf.n;
  const size_t m = std::min(cap, (size_t)kf.n);
  if (m == 0) return GICP_OK;
  HIP_TRY(hipSetDevice(o->device));
  return read_xyz(nullptr, kf.pts.as<float4>(), m, xyz);   // the null stream (idle: process waited for the keyframe)
}

gicp_status ddlo_odom_keyframe_points_xyzi(const ddlo_odom* o, int k, float* xyzi, size_t cap, size_t* n) {
  if (!o || !n || (!xyzi && cap) || k < 0 || k >= (int)o->keyframes.size()) return fail(GICP_EINVAL, "invalid argument");
  if (!o->inten_use) return fail(GICP_EINVAL, "the driver carries no intensity (ddlo_odom_set_intensity)");
  const Keyframe& kf = *o->keyframes[k];
  *n = (size_t)kf.n;
  const size_t m = std::min(cap, (size_t)kf.n);
  if (m == 0) return GICP_OK;
  HIP_TRY(hipSetDevice(o->device));
  HIP_TRY(hipMemcpy(xyzi, kf.pts.p, sizeof(float4) * m, hipMemcpyDeviceToHost));   // (idle, as ddlo_odom_keyframe_points)
  return GICP_OK;
}

gicp_status ddlo_odom_set_intensity(ddlo_odom* o, int use, size_t offset_bytes) {
  if (!o) return fail(GICP_EINVAL, "null handle");
  if ((use != 0) != (o->inten_use != 0) && !o->keyframes.empty())
    return fail(GICP_EINVAL, "intensity: a driver's keyframes either all have the channel or none do");
  o->inten_use = use != 0;
  o->inten_off = use ? offset_bytes : 0;
  return GICP_OK;
}

gicp_status ddlo_odom_get_intensity(const ddlo_odom* o, int* use, size_t* offset_bytes) {
  if (!o) return fail(GICP_EINVAL, "null handle");
  if (use) *use = o->inten_use;
  if (offset_bytes) *offset_bytes = o->inten_off;
  return GICP_OK;
}

gicp_status ddlo_odom_set_deskew(ddlo_odom* o, const ddlo_deskew_params* p) {
  if (!o || !p) return fail(GICP_EINVAL, "null argument");
  if (p->time_type < DDLO_TIME_F32_S || p->time_type > DDLO_TIME_F64_S) return fail(GICP_EINVAL, "deskew: unknown time type");
  if (!std::isfinite(p->period) || !(p->period > 0)) return fail(GICP_EINVAL, "deskew: the period must be finite and > 0");
  if (!std::isfinite(p->ref_time)) return fail(GICP_EINVAL, "deskew: non-finite reference time");
  o->dk = *p;
  o->dk.use = p->use != 0;
  return GICP_OK;
}

gicp_status ddlo_odom_get_deskew(const ddlo_odom* o, ddlo_deskew_params* p) {
  if (!o || !p) return fail(GICP_EINVAL, "null argument");
  *p = o->dk;
  return GICP_OK;
}

gicp_status ddlo_odom_set_deskew_motion(ddlo_odom* o, const double omega[3], const double t[3]) {
  if (!o) return fail(GICP_EINVAL, "null handle");
  if (!omega || !t) {
    o->dk_pending = false;
    return GICP_OK;
  }
  for (int a = 0; a < 3; ++a)
    if (!std::isfinite(omega[a]) || !std::isfinite(t[a])) return fail(GICP_EINVAL, "deskew: non-finite twist");
  std::memcpy(o->dk_pend_w, omega, sizeof(o->dk_pend_w));
  std::memcpy(o->dk_pend_t, t, sizeof(o->dk_pend_t));
  o->dk_pending = true;
  return GICP_OK;
}

gicp_status ddlo_odom_deskew_motion(const ddlo_odom* o, double omega[3], double t[3], int* source) {
  if (!o) return fail(GICP_EINVAL, "null handle");
  for (int a = 0; a < 3; ++a) {
    if (omega) omega[a] = o->dk_source ? o->dk_w[a] : 0.0;
    if (t) t[a] = o->dk_source ? o->dk_t[a] : 0.0;
  }
  if (source) *source = o->dk_source;
  return GICP_OK;
}

gicp_status ddlo_odom_keyframe(const ddlo_odom* o, int k, float pose7[7], size_t* npoints) {
  if (!o || k < 0 || k >= (int)o->keyframes.size()) return fail(GICP_EINVAL, "invalid keyframe index");
  const Keyframe& kf = *o->keyframes[k];
  if (pose7) {
    pose7[0] = kf.pose[0];
    pose7[1] = kf.pose[1];
    pose7[2] = kf.pose[2];
    pose7[3] = kf.q.x;
    pose7[4] = kf.q.y;
    pose7[5] = kf.q.z;
    pose7[6] = kf.q.w;
  }
  if (npoints) *npoints = (size_t)kf.n;
  return GICP_OK;
}

gicp_status ddlo_odom_submap(const ddlo_odom* o, int32_t* idx, size_t cap, size_t* n) {
  if (!o || !n) return fail(GICP_EINVAL, "null argument");
  *n = o->submap_prev.size();
  if (idx)
    for (size_t i = 0; i < std::min(cap, o->submap_prev.size()); ++i) idx[i] = o->submap_prev[i];
  return GICP_OK;
}

gicp_status ddlo_odom_ctx(ddlo_odom* o, int which, gicp_ctx** ctx) {
  if (!o || !ctx || (which != 0 && which != 1)) return fail(GICP_EINVAL, "invalid argument");
  *ctx = which == 0 ? o->s2s : o->s2m;
  return GICP_OK;
}

gicp_status ddlo_odom_set_voxel_order(ddlo_odom* o, int order) {
  if (!o) return fail(GICP_EINVAL, "null handle");
  if (order != DDLO_VOXEL_ORDER_INPUT && order != DDLO_VOXEL_ORDER_PCL) return fail(GICP_EINVAL, "unknown voxel order");
  o->voxel_order = order;
  return GICP_OK;
}

gicp_status ddlo_odom_get_voxel_order(const ddlo_odom* o, int* order) {
  if (!o || !order) return fail(GICP_EINVAL, "null argument");
  *order = o->voxel_order;
  return GICP_OK;
}

gicp_status ddlo_preprocess(int device, const float* xyz, size_t n, size_t stride, double crop_size, double leaf,
                            float* out, size_t cap, size_t* nout) {
  return ddlo_preprocess_ordered(device, xyz, n, stride, crop_size, leaf, DDLO_VOXEL_ORDER_INPUT, out, cap, nout);
}

gicp_status ddlo_odom_set_downsampling(ddlo_odom* o, int use, int row_step, int col_step, int rows, int cols) {
  if (!o) return fail(GICP_EINVAL, "null handle");
  if (row_step < 1 || col_step < 1 || rows < 1 || cols < 1 || (long long)rows * cols > INT32_MAX / 2)
    return fail(GICP_EINVAL, "downsampling: steps, rows and cols must be >= 1");
  o->ds_use = use != 0;
  o->ds_row = row_step;
  o->ds_col = col_step;
  o->ds_rows = rows;
  o->ds_cols = cols;
  return GICP_OK;
}

gicp_status ddlo_odom_get_downsampling(const ddlo_odom* o, int* use, int* row_step, int* col_step, int* rows, int* cols) {
  if (!o) return fail(GICP_EINVAL, "null handle");
  if (use) *use = o->ds_use;
  if (row_step) *row_step = o->ds_row;
  if (col_step) *col_step = o->ds_col;
  if (rows) *rows = o->ds_rows;
  if (cols) *cols = o->ds_cols;
  return GICP_OK;
}

// ddlo_preprocess_ordered / ddlo_preprocess_downsampled (rows > 0: through the row/column filter)
static gicp_status preprocess_entry(int device, const float* xyz, size_t n, size_t stride, int rows, int cols, int row_step,
                                    int col_step, double crop_size, double leaf, int order, float* out, size_t cap,
                                    size_t* nout, bool intensity = false, size_t ioff = 0) {
  if ((!xyz && n) || !nout || stride < 12 || stride % 4 || n > (size_t)INT32_MAX / 2) return fail(GICP_EINVAL, "invalid argument");
  if (intensity && !intensity_offset_ok(ioff, stride))
    return fail(GICP_EINVAL, "intensity offset: a multiple of 4, >= 12 and offset + 4 <= stride");
  if (order != DDLO_VOXEL_ORDER_INPUT && order != DDLO_VOXEL_ORDER_PCL) return fail(GICP_EINVAL, "unknown voxel order");
  ddlo_odom_params p;
  ddlo_odom_default_params(&p);
  ddlo_odom* o = nullptr;
  gicp_status st = ddlo_odom_create(device, &p, &o);
  if (st) return st;
  std::unique_ptr<ddlo_odom, gicp_status (*)(ddlo_odom*)> guard(o, ddlo_odom_destroy);
  o->voxel_order = order;
  o->inten_use = intensity;
  o->inten_off = intensity ? ioff : 0;
  if (rows > 0) {
    st = ddlo_odom_set_downsampling(o, 1, row_step, col_step, rows, cols);
    if (st) return st;
  }
  *nout = 0;
  if (n == 0) return GICP_OK;
  const size_t raw = raw_bytes(n, stride, o->inten_off);
  HIP_TRY(o->up.ensure(raw));
  HIP_TRY(hipMemcpyAsync(o->up.p, xyz, raw, hipMemcpyHostToDevice, o->s));
  HIP_TRY(o->a.ensure(sizeof(float4) * n));
  const int nr = pack_scan(o, (int)n, stride);
  int m = 0;
  st = preprocess(o, nr, crop_size > 0, crop_size, leaf > 0, leaf, &m);
  if (st) return st;
  *nout = (size_t)m;
  if (out && m > 0) {
    if ((size_t)m > cap) return fail(GICP_EINVAL, "output capacity too small");
    if (intensity) {   // 16 B per point, as they lie
      HIP_TRY(hipMemcpyAsync(out, o->a.p, sizeof(float4) * (size_t)m, hipMemcpyDeviceToHost, o->s));
      HIP_TRY(hipStreamSynchronize(o->s));
      return GICP_OK;
    }
    return read_xyz(o->s, o->a.as<float4>(), (size_t)m, out);
  }
  return GICP_OK;
}

gicp_status ddlo_preprocess_xyzi(int device, const float* pts, size_t n, size_t stride, size_t offset_bytes,
                                 double crop_size, double leaf, int order, float* out_xyzi, size_t cap, size_t* n_out) {
  return preprocess_entry(device, pts, n, stride, 0, 0, 1, 1, crop_size, leaf, order, out_xyzi, cap, n_out, true,
                          offset_bytes);
}

gicp_status ddlo_preprocess_ordered(int device, const float* xyz, size_t n, size_t stride, double crop_size, double leaf,
                                    int order, float* out, size_t cap, size_t* nout) {
  return preprocess_entry(device, xyz, n, stride, 0, 0, 1, 1, crop_size, leaf, order, out, cap, nout);
}

gicp_status ddlo_preprocess_downsampled(int device, const float* xyz, size_t n, size_t stride, int rows, int cols,
                                        int row_step, int col_step, double crop_size, double leaf, int order, float* out,
                                        size_t cap, size_t* nout) {
  if (rows < 1 || cols < 1 || row_step < 1 || col_step < 1)
    return fail(GICP_EINVAL, "downsampling: steps, rows and cols must be >= 1");
  return preprocess_entry(device, xyz, n, stride, rows, cols, row_step, col_step, crop_size, leaf, order, out, cap, nout);
}

gicp_status ddlo_median_range(int device, const float* xyz, size_t n, size_t stride, float* median) {
  if ((!xyz && n) || !median || stride < 12 || stride % 4 || n > (size_t)INT32_MAX / 2) return fail(GICP_EINVAL, "invalid argument");
  ddlo_odom_params p;
  ddlo_odom_default_params(&p);
  ddlo_odom* o = nullptr;
  gicp_status st = ddlo_odom_create(device, &p, &o);
  if (st) return st;
  std::unique_ptr<ddlo_odom, gicp_status (*)(ddlo_odom*)> guard(o, ddlo_odom_destroy);
  *median = 0.f;
  if (n == 0) return GICP_OK;
  HIP_TRY(o->up.ensure((n - 1) * stride + 12));
  HIP_TRY(hipMemcpyAsync(o->up.p, xyz, (n - 1) * stride + 12, hipMemcpyHostToDevice, o->s));
  HIP_TRY(o->a.ensure(sizeof(float4) * n));
  launch_pack4(o->s, o->up.as<unsigned char>(), stride, (int)n, o->a.as<float4>());
  HIP_TRY(o->rng.ensure(sizeof(float) * n));
  HIP_TRY(o->rng_sorted.ensure(sizeof(float) * n));
  HIP_TRY(o->medtmp.ensure(median_tmp_bytes((int)n)));
  median_range_async(o->s, o->a.as<float4>(), (int)n, o->rng.as<float>(), o->rng_sorted.as<float>(), o->medtmp.p,
                     o->medtmp.bytes, o->median_pin.as<float>());
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipStreamSynchronize(o->s));
  *median = *o->median_pin.as<float>();
  return GICP_OK;
}

gicp_status ddlo_convex_hull(const float* xyz, int n, int32_t* idx, int cap, int* nidx) {
  if ((!xyz && n) || (!idx && cap > 0) || !nidx || n < 0 || cap < 0) return fail(GICP_EINVAL, "invalid argument");
  const std::vector<int> h = convex_hull(xyz, n);
  for (size_t i = 0; i < h.size() && (int)i < cap; ++i) idx[i] = h[i];
  *nidx = (int)h.size();
  return GICP_OK;
}

gicp_status ddlo_concave_hull(const float* xyz, int n, double alpha, int32_t* idx, int cap, int* nidx) {
  if ((!xyz && n) || (!idx && cap > 0) || !nidx || n < 0 || cap < 0) return fail(GICP_EINVAL, "invalid argument");
  const std::vector<int> h = concave_hull(xyz, n, alpha);
  for (size_t i = 0; i < h.size() && (int)i < cap; ++i) idx[i] = h[i];
  *nidx = (int)h.size();
  return GICP_OK;
}

}  // extern "C"

// odom_internal.hpp: keyframe k's cloud where it lives (the global map reads it device to device)
gicp_status ddlo::odom_keyframe_dev(const ddlo_odom* o, int k, const float4** pts, int* n, int* device,
                                    hipStream_t* stream) {
  if (!o || !pts || !n || !device || !stream || k < 0 || k >= (int)o->keyframes.size())
    return fail(GICP_EINVAL, "invalid keyframe index");
  const Keyframe& kf = *o->keyframes[k];
  *pts = kf.pts.as<float4>();
  *n = kf.n;
  *device = o->device;
  *stream = o->s;
  return GICP_OK;
}

bool ddlo::odom_has_intensity(const ddlo_odom* o) { return o && o->inten_use != 0; }
