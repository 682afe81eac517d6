// track_core.hpp — the object tracker, host only, STL only (a stand-alone
// program can compile it: tests/cpp/track_replay.cpp).  A literal restatement of
//   TrackingModule      src/tracking/tracking.cpp
//   BoundingBoxFilter   src/tracking/bounding_box_filter.cpp
//   KalmanFilter        src/tracking/kalman.cpp
//   HungarianAlgorithm  src/tracking/hungarian.cpp (Buehren's Munkres)
//   OBBIoU              include/util/bbox_iou.h
// of the reference (dynamic_direct_lidar_odometry/).  Compile with
// -ffp-contract=off: the IoU is float arithmetic whose every product and sum
// rounds on its own, the Kalman filter double arithmetic likewise.
#pragma once

#include <cfloat>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <utility>
#include <vector>

namespace ddlo {
namespace trk {

enum Status { UNDEFINED = 0, STATIC = 1, DYNAMIC = 2 };   // object.h:9-14

struct Params {                   // tracking.h:33-38
  size_t max_no_hits = 30;
  size_t min_dynamic_hits = 5;
  size_t max_undefined_hits = 1;
  float max_obj_velocity = 15.f;
  double min_travel_dist = 0.75;
  double res_height_ratio = 0.3;
};

struct Detection {                // Object (object.h:16-26) as getObject fills it (detection.cpp:726-782)
  int id = -1;
  double state[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};   // entries 7..9: 0 (the reference leaves them unset)
  int num_points = 0;
  float avg_residuum = 0.f;
  int status = UNDEFINED;
};

struct Box {                      // the jsk BoundingBox fields updateBBoxHistory fills (:223-233)
  double position[3];
  double orientation_z;
  double dimensions[3];
};

// ---- bbox_iou.h, in float ----
namespace iou {

struct Vec {
  float x, y;
  Vec operator+(const Vec& o) const { return Vec{x + o.x, y + o.y}; }
  float cross(const Vec& o) const { return x * o.y - y * o.x; }   // :22-25
};

struct Line {                     // :34-55
  float a, b, c;
  Line(const Vec& v1, const Vec& v2) : a(v2.y - v1.y), b(v1.x - v2.x), c(v2.cross(v1)) {}
  float call(const Vec& p) const { return a * p.x + b * p.y + c; }
  Vec intersection(const Line& o) const {
    const float w = a * o.b - b * o.a;
    return Vec{(b * o.c - c * o.b) / w, (c * o.a - a * o.c) / w};
  }
};

// rectangle_vertices (:57-73): r is used as an angle in radians; the caller
// passes state[3] = sin(yaw / 2) there (OBBIoU :136-137), restated as it is
inline void rectangle_vertices(float cx, float cy, float w, float h, float r, Vec out[4]) {
  const float angle = r;
  const float dx = (float)(w / 2.0);
  const float dy = (float)(h / 2.0);
  const float dxcos = dx * cosf(angle);
  const float dxsin = dx * sinf(angle);
  const float dycos = dy * cosf(angle);
  const float dysin = dy * sinf(angle);
  const Vec c{cx, cy};
  out[0] = c + Vec{-dxcos - -dysin, -dxsin + -dycos};
  out[1] = c + Vec{dxcos - -dysin, dxsin + -dycos};
  out[2] = c + Vec{dxcos - dysin, dxsin + dycos};
  out[3] = c + Vec{-dxcos - dysin, -dxsin + dycos};
}

// intersection_area (:75-129)
inline double intersection_area(float cx1, float cy1, float w1, float h1, float r1, float cx2, float cy2, float w2,
                                float h2, float r2) {
  Vec rect1[4], rect2[4];
  rectangle_vertices(cx1, cy1, w1, h1, r1, rect1);
  rectangle_vertices(cx2, cy2, w2, h2, r2, rect2);
  std::vector<Vec> inter(rect1, rect1 + 4), next;
  std::vector<float> line_values;
  for (int i = 0; i < 4; ++i) {
    if (inter.size() <= 2) break;
    const Vec p = rect2[i], q = rect2[(i + 1) % 4];
    const Line line(p, q);
    next.clear();
    line_values.clear();
    for (size_t j = 0; j < inter.size(); ++j) line_values.push_back(line.call(inter[j]));
    for (size_t k = 0; k < inter.size(); ++k) {
      const float s_value = line_values[k];
      const float t_value = line_values[(k + 1) % inter.size()];
      const Vec s = inter[k], t = inter[(k + 1) % inter.size()];
      if (s_value <= 0.0) next.push_back(s);
      if (s_value * t_value < 0) next.push_back(line.intersection(Line(s, t)));
    }
    inter = next;
  }
  if (inter.size() <= 2) return 0.0;
  float area_sum = 0.0;
  for (size_t i = 0; i < inter.size(); ++i) {
    const Vec p = inter[i], q = inter[(i + 1) % inter.size()];
    area_sum += p.x * q.y - p.y * q.x;
  }
  return 0.5 * area_sum;
}

// std::max / std::min as <algorithm> defines them: the argument order decides what a NaN does
inline float max_f(float a, float b) { return (a < b) ? b : a; }
inline float min_f(float a, float b) { return (b < a) ? b : a; }

// OBBIoU (:131-157) over two 7-states
inline double obb_iou(const double* s1, const double* s2) {
  float b1[7], b2[7];
  for (int i = 0; i < 7; ++i) {
    b1[i] = (float)s1[i];
    b2[i] = (float)s2[i];
  }
  const double inter = intersection_area(b1[0], b1[1], b1[4], b1[5], b1[3], b2[0], b2[1], b2[4], b2[5], b2[3]);
  const float min_1 = (float)(b1[2] - b1[6] / 2.0);
  const float min_2 = (float)(b2[2] - b2[6] / 2.0);
  const float max_1 = (float)(b1[2] + b1[6] / 2.0);
  const float max_2 = (float)(b2[2] + b2[6] / 2.0);
  const float max_min = max_f(min_1, min_2);
  const float min_max = min_f(max_1, max_2);
  const float height_overlap = max_f(min_max - max_min, 0.0f);
  const float intersection_volume = (float)(height_overlap * inter);
  const float total_volume = b1[4] * b1[5] * b1[6] + b2[4] * b2[5] * b2[6] - intersection_volume;
  const float ratio = intersection_volume / total_volume;
  // deviation: two zero-volume boxes give 0 / 0, a NaN cost on which the
  // reference's Hungarian solver never returns; the pair's IoU is 0 here
  if (ratio != ratio) return 0.0;
  float v = max_f(ratio, 0.0f);
  v = min_f(v, 1.0f);
  return v;
}

}  // namespace iou

// ---- hungarian.cpp: assignmentoptimal (:83-210) and its steps, column-major
// working copy, the recursion of step2a .. step5 unrolled into one loop ----
inline void hungarian(const double* cost_rm, int nRows, int nCols, int* assignment) {
  for (int r = 0; r < nRows; ++r) assignment[r] = -1;
  const int nEl = nRows * nCols;
  if (nEl <= 0) return;
  std::vector<double> dist((size_t)nEl);
  for (int i = 0; i < nRows; ++i)          // Solve :64-66: distMatrixIn[i + nRows * j]
    for (int j = 0; j < nCols; ++j) dist[(size_t)i + (size_t)nRows * j] = cost_rm[(size_t)i * nCols + j];
  std::vector<char> coveredColumns(nCols, 0), coveredRows(nRows, 0), star(nEl, 0), prime(nEl, 0), newStar(nEl, 0);
  int minDim;
  auto zero = [&](int row, int col) { return std::fabs(dist[(size_t)row + (size_t)nRows * col]) < DBL_EPSILON; };
  if (nRows <= nCols) {                    // :117-154
    minDim = nRows;
    for (int row = 0; row < nRows; ++row) {
      double minValue = dist[row];
      for (int col = 1; col < nCols; ++col) {
        const double value = dist[(size_t)row + (size_t)nRows * col];
        if (value < minValue) minValue = value;
      }
      for (int col = 0; col < nCols; ++col) dist[(size_t)row + (size_t)nRows * col] -= minValue;
    }
    for (int row = 0; row < nRows; ++row)
      for (int col = 0; col < nCols; ++col)
        if (zero(row, col))
          if (!coveredColumns[col]) {
            star[(size_t)row + (size_t)nRows * col] = 1;
            coveredColumns[col] = 1;
            break;
          }
  } else {                                 // :155-192
    minDim = nCols;
    for (int col = 0; col < nCols; ++col) {
      double* c = dist.data() + (size_t)nRows * col;
      double minValue = c[0];
      for (int row = 1; row < nRows; ++row)
        if (c[row] < minValue) minValue = c[row];
      for (int row = 0; row < nRows; ++row) c[row] -= minValue;
    }
    for (int col = 0; col < nCols; ++col)
      for (int row = 0; row < nRows; ++row)
        if (zero(row, col))
          if (!coveredRows[row]) {
            star[(size_t)row + (size_t)nRows * col] = 1;
            coveredColumns[col] = 1;
            coveredRows[row] = 1;
            break;
          }
    for (int row = 0; row < nRows; ++row) coveredRows[row] = 0;
  }
  // step2b (:272-295), then step3 (:298-342), step4 (:345-399) -> step2a
  // (:244-269) -> step2b, or step5 (:402-436) -> step3
  for (;;) {
    int nCovered = 0;
    for (int col = 0; col < nCols; ++col)
      if (coveredColumns[col]) ++nCovered;
    if (nCovered == minDim) break;
    // step3 until it reaches step4
    int prow = -1, pcol = -1;
    for (;;) {
      bool to_step4 = false, zerosFound = true;
      while (zerosFound && !to_step4) {
        zerosFound = false;
        for (int col = 0; col < nCols && !to_step4; ++col)
          if (!coveredColumns[col])
            for (int row = 0; row < nRows; ++row)
              if (!coveredRows[row] && zero(row, col)) {
                prime[(size_t)row + (size_t)nRows * col] = 1;
                int starCol = 0;
                for (; starCol < nCols; ++starCol)
                  if (star[(size_t)row + (size_t)nRows * starCol]) break;
                if (starCol == nCols) {
                  prow = row;
                  pcol = col;
                  to_step4 = true;
                } else {
                  coveredRows[row] = 1;
                  coveredColumns[starCol] = 0;
                  zerosFound = true;
                }
                break;
              }
      }
      if (to_step4) break;
      // step5
      double h = DBL_MAX;
      for (int row = 0; row < nRows; ++row)
        if (!coveredRows[row])
          for (int col = 0; col < nCols; ++col)
            if (!coveredColumns[col]) {
              const double value = dist[(size_t)row + (size_t)nRows * col];
              if (value < h) h = value;
            }
      // (no uncovered element compares below DBL_MAX: only a NaN / inf matrix
      // gets here, where the reference recurses without end; the stars stand)
      if (!(h < DBL_MAX)) goto done;
      for (int row = 0; row < nRows; ++row)
        if (coveredRows[row])
          for (int col = 0; col < nCols; ++col) dist[(size_t)row + (size_t)nRows * col] += h;
      for (int col = 0; col < nCols; ++col)
        if (!coveredColumns[col])
          for (int row = 0; row < nRows; ++row) dist[(size_t)row + (size_t)nRows * col] -= h;
    }
    // step4
    newStar = star;
    newStar[(size_t)prow + (size_t)nRows * pcol] = 1;
    int starCol = pcol, starRow = 0;
    for (; starRow < nRows; ++starRow)
      if (star[(size_t)starRow + (size_t)nRows * starCol]) break;
    while (starRow < nRows) {
      newStar[(size_t)starRow + (size_t)nRows * starCol] = 0;
      const int primeRow = starRow;
      int primeCol = 0;
      for (; primeCol < nCols; ++primeCol)
        if (prime[(size_t)primeRow + (size_t)nRows * primeCol]) break;
      newStar[(size_t)primeRow + (size_t)nRows * primeCol] = 1;
      starCol = primeCol;
      for (starRow = 0; starRow < nRows; ++starRow)
        if (star[(size_t)starRow + (size_t)nRows * starCol]) break;
    }
    for (int n = 0; n < nEl; ++n) {
      prime[n] = 0;
      star[n] = newStar[n];
    }
    for (int n = 0; n < nRows; ++n) coveredRows[n] = 0;
    // step2a
    for (int col = 0; col < nCols; ++col)
      for (int row = 0; row < nRows; ++row)
        if (star[(size_t)row + (size_t)nRows * col]) {
          coveredColumns[col] = 1;
          break;
        }
  }
done:
  // buildassignmentvector (:213-228)
  for (int row = 0; row < nRows; ++row)
    for (int col = 0; col < nCols; ++col)
      if (star[(size_t)row + (size_t)nRows * col]) {
        assignment[row] = col;
        break;
      }
}

// ---- kalman.cpp:69-92 with the matrices of bounding_box_filter.cpp:15-37,55-58,
// dense, every product and sum rounded on its own, sums in index order ----
constexpr int KN = 10, KM = 7;

struct Kalman {
  double x[KN];
  double P[KN][KN];

  void init(const double* x0) {            // P0: :28-30
    for (int i = 0; i < KN; ++i) {
      x[i] = x0[i];
      for (int j = 0; j < KN; ++j) P[i][j] = 0.0;
      P[i][i] = i < KM ? 1000.0 : 10000.0;
    }
  }
  static double A_at(int i, int j, double dt) { return i == j ? 1.0 : (i < 3 && j == i + 7 ? dt : 0.0); }   // :56-58
  static double C_at(int i, int j) { return i == j ? 1.0 : 0.0; }                                            // :25-26
  static double Q_at(int i, int j) { return i != j ? 0.0 : (i < KM ? 1.0 : .01); }                            // :35-37

  void predict(double dt) {                // kalman.cpp:69-81
    double xn[KN], AP[KN][KN];
    for (int i = 0; i < KN; ++i) {
      double s = 0.0;
      for (int k = 0; k < KN; ++k) s += A_at(i, k, dt) * x[k];
      xn[i] = s;
    }
    for (int i = 0; i < KN; ++i)
      for (int j = 0; j < KN; ++j) {
        double s = 0.0;
        for (int k = 0; k < KN; ++k) s += A_at(i, k, dt) * P[k][j];
        AP[i][j] = s;
      }
    for (int i = 0; i < KN; ++i)
      for (int j = 0; j < KN; ++j) {
        double s = 0.0;
        for (int k = 0; k < KN; ++k) s += AP[i][k] * A_at(j, k, dt);
        P[i][j] = s + Q_at(i, j);
      }
    for (int i = 0; i < KN; ++i) x[i] = xn[i];
  }

  void update(const double* y) {           // kalman.cpp:83-92; y: the first KM entries of the detection's state
    double PCt[KN][KM], S[KM][KM], K[KN][KM], KC[KN][KN], Pn[KN][KN];
    for (int i = 0; i < KN; ++i)
      for (int j = 0; j < KM; ++j) {
        double s = 0.0;
        for (int k = 0; k < KN; ++k) s += P[i][k] * C_at(j, k);
        PCt[i][j] = s;
      }
    for (int i = 0; i < KM; ++i)
      for (int j = 0; j < KM; ++j) {
        double s = 0.0;
        for (int k = 0; k < KN; ++k) s += C_at(i, k) * PCt[k][j];
        S[i][j] = s + (i == j ? 1.0 : 0.0);   // R: :32-33
      }
    // (C P C^T + R) is diagonal (A, Q, P0 couple only (x, vx), (y, vy), (z, vz)): its inverse is 1 / s_ii
    for (int i = 0; i < KN; ++i)
      for (int j = 0; j < KM; ++j) K[i][j] = PCt[i][j] * (1.0 / S[j][j]);
    for (int i = 0; i < KN; ++i) {
      double s = 0.0;
      for (int j = 0; j < KM; ++j) {
        double cx = 0.0;
        for (int k = 0; k < KN; ++k) cx += C_at(j, k) * x[k];
        s += K[i][j] * (y[j] - cx);
      }
      KC[i][0] = s;   // (scratch: the state's increment)
    }
    double xn[KN];
    for (int i = 0; i < KN; ++i) xn[i] = x[i] + KC[i][0];
    for (int i = 0; i < KN; ++i)
      for (int j = 0; j < KN; ++j) {
        double s = 0.0;
        for (int k = 0; k < KM; ++k) s += K[i][k] * C_at(k, j);
        KC[i][j] = s;
      }
    for (int i = 0; i < KN; ++i)
      for (int j = 0; j < KN; ++j) {
        double s = 0.0;
        for (int k = 0; k < KN; ++k) s += ((i == k ? 1.0 : 0.0) - KC[i][k]) * P[k][j];
        Pn[i][j] = s;
      }
    for (int i = 0; i < KN; ++i) {
      x[i] = xn[i];
      for (int j = 0; j < KN; ++j) P[i][j] = Pn[i][j];
    }
  }
};

// ---- BoundingBoxFilter ----
struct Filter {
  int filter_id = 0;
  size_t hits = 1;                         // bounding_box_filter.h:50
  size_t sslu = 0;                         // steps_since_last_update_
  Detection obj;                           // tracked_object_
  Kalman kf;
  double first_pose[3] = {0, 0, 0};        // first_pose_.pose.position
  double current_pose[3] = {0, 0, 0};      // current_pose_.pose.position (zero until the first update)
  std::vector<Box> static_bboxes;
  bool has_turned_dynamic = false;

  Filter(const Detection& d, int id) : filter_id(id), obj(d) {   // :3-51
    double x0[KN];
    for (int i = 0; i < 7; ++i) x0[i] = d.state[i];
    x0[7] = x0[8] = x0[9] = 0.0;
    kf.init(x0);
    first_pose[0] = x0[0];
    first_pose[1] = x0[1];
    first_pose[2] = x0[2];
  }

  void predict(double dt) {                // :53-62
    kf.predict(dt);
    ++sslu;
  }

  const Detection& get_object() {          // :87-91
    for (int i = 0; i < KN; ++i) obj.state[i] = kf.x[i];
    return obj;
  }

  void update(const Detection& d, const Params& p) {   // :64-85
    ++hits;
    sslu = 0;
    const int old_status = obj.status;
    obj = d;
    obj.status = old_status;
    current_pose[0] = obj.state[0];
    current_pose[1] = obj.state[1];
    current_pose[2] = obj.state[2] - obj.state[6] / 2;   // bottom of bbox
    update_dynamic_status(p);
    update_bbox_history();
    kf.update(obj.state);
  }

  void update_dynamic_status(const Params& p) {   // :169-217
    switch (obj.status) {
      case DYNAMIC:
        has_turned_dynamic = false;
        break;
      case UNDEFINED:
        if (hits > p.max_undefined_hits) {
          obj.status = STATIC;
          break;
        }
        if (hits < p.min_dynamic_hits) break;
        // falls through: the STATIC check (a direct transition to DYNAMIC is possible)
      case STATIC: {
        const float min_required_residuum = (float)(obj.state[6] * p.res_height_ratio);
        if (obj.avg_residuum < min_required_residuum) return;
        const double x0 = first_pose[0], y0 = first_pose[1];
        const double x = current_pose[0], y = current_pose[1];
        const double d_squared = (x - x0) * (x - x0) + (y - y0) * (y - y0);
        if (d_squared >= p.min_travel_dist * p.min_travel_dist) {
          obj.status = DYNAMIC;
          has_turned_dynamic = !static_bboxes.empty();
        }
        break;
      }
    }
  }

  void update_bbox_history() {             // :219-243
    if (obj.status != STATIC) return;
    Box b;
    b.position[0] = obj.state[0];
    b.position[1] = obj.state[1];
    b.position[2] = obj.state[2];
    b.orientation_z = obj.state[3];
    b.dimensions[0] = obj.state[4];
    b.dimensions[1] = obj.state[5];
    b.dimensions[2] = obj.state[6];
    static_bboxes.push_back(b);
    if (static_bboxes.size() > 5) static_bboxes.erase(static_bboxes.begin());
  }

  bool take_static_bboxes(std::vector<Box>& out) {   // getStaticBBoxes :157-167
    if (!has_turned_dynamic) return false;
    out.insert(out.end(), static_bboxes.begin(), static_bboxes.end());
    has_turned_dynamic = false;
    static_bboxes.clear();
    return true;
  }

  double dist_to_origin() const {          // :245-252
    if (hits < 2) return 0;
    const double dx = current_pose[0] - first_pose[0], dy = current_pose[1] - first_pose[1],
                 dz = current_pose[2] - first_pose[2];
    return std::sqrt(dx * dx + dy * dy + dz * dz);
  }
};

// ---- TrackingModule ----
struct Tracker {
  Params p;
  int next_id = 0;                         // filter_id_
  std::vector<Filter> filters;
  std::vector<int> assignment;
  std::vector<std::pair<int, int>> matches;
  std::vector<int> unmatched_detections, unmatched_states;
  // the last associate()'s matrices (rows = detections, cols = filters) and the
  // last update's by-products
  std::vector<double> cost;
  std::vector<float> disp;
  int rows = 0, cols = 0;
  std::vector<int> track_of_detection, erased;
  std::vector<Box> cleared;                // collected until taken
  int turned_dynamic = 0, boxes_collected = 0;

  static double cost_simple(const Detection& d, const Detection& t) {   // getCostSimple :152-161
    return std::sqrt((d.state[0] - t.state[0]) * (d.state[0] - t.state[0]) +
                     (d.state[1] - t.state[1]) * (d.state[1] - t.state[1]) +
                     (d.state[2] - t.state[2]) * (d.state[2] - t.state[2]));
  }

  static double cost_full(const Detection& d, const Detection& t) {     // getCostFull :172-190
    const double bbox_cost = 1 - iou::obb_iou(d.state, t.state);
    const float np_det = (float)d.num_points;
    const float np_track = (float)t.num_points;
    const float point_diff_rel_inv = (np_track >= np_det) ? np_det / np_track : np_track / np_det;
    const float point_diff_rel = 1 - point_diff_rel_inv;
    const float beta = 0.8;
    const float gamma = 0.1;
    return beta * bbox_cost + gamma * point_diff_rel;
  }

  void associate(const std::vector<Detection>& dets, const std::vector<Detection>& tracked, float dt) {   // :80-150
    rows = cols = 0;
    cost.clear();
    disp.clear();
    assignment.clear();
    if (tracked.empty()) {
      unmatched_detections.resize(dets.size());
      for (size_t i = 0; i < dets.size(); ++i) unmatched_detections[i] = (int)i;
      return;
    }
    if (dets.empty()) return;
    rows = (int)dets.size();
    cols = (int)tracked.size();
    for (int i = 0; i < rows; ++i)
      for (int j = 0; j < cols; ++j) {
        cost.push_back(cost_full(dets[i], tracked[j]));
        disp.push_back((float)cost_simple(dets[i], tracked[j]));
      }
    assignment.assign(rows, -1);
    hungarian(cost.data(), rows, cols, assignment.data());
    for (int i = 0; i < rows; ++i) {
      if (assignment[i] != -1) matches.push_back(std::make_pair(i, assignment[i]));
      else unmatched_detections.push_back(i);
    }
    for (int i = 0; i < cols; ++i) {
      bool found = false;
      for (int a : assignment) found = found || a == i;
      if (!found) unmatched_states.push_back(i);
    }
    for (auto it = matches.begin(); it != matches.end();) {
      if (disp[(size_t)it->first * cols + it->second] > p.max_obj_velocity * dt) {
        unmatched_detections.push_back(it->first);
        unmatched_states.push_back(it->second);
        it = matches.erase(it);
      } else {
        ++it;
      }
    }
  }

  void update(float dt, const std::vector<Detection>& dets) {   // :27-78 (dt is a float there)
    matches.clear();
    unmatched_detections.clear();
    unmatched_states.clear();
    std::vector<Detection> tracked;
    for (Filter& f : filters) {
      f.predict(dt);
      tracked.push_back(f.get_object());
    }
    associate(dets, tracked, dt);
    track_of_detection.assign(dets.size(), -1);
    for (auto& m : matches) {
      filters[m.second].update(dets[m.first], p);
      track_of_detection[m.first] = filters[m.second].filter_id;
    }
    for (int det : unmatched_detections) {
      filters.emplace_back(dets[det], next_id);
      track_of_detection[det] = next_id;
      ++next_id;
    }
    erased.clear();
    for (auto it = filters.begin(); it != filters.end();) {
      if ((size_t)(int)it->sslu >= p.max_no_hits) {
        erased.push_back(it->filter_id);
        it = filters.erase(it);
      } else {
        ++it;
      }
    }
    // publishBBoxes :259-275
    turned_dynamic = 0;
    const size_t before = cleared.size();
    for (Filter& f : filters)
      if (f.take_static_bboxes(cleared)) ++turned_dynamic;
    boxes_collected = (int)(cleared.size() - before);
  }

  size_t count(int mask) const {
    size_t c = 0;
    for (const Filter& f : filters) c += (mask >> f.obj.status) & 1;
    return c;
  }
};

}  // namespace trk
}  // namespace ddlo
