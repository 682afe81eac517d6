// track.hip — the C-ABI of the object tracker (include/ddlo_track.h) over
// track_core.hpp.  Host code only: no kernel, no HIP call, no device.
#include <cmath>
#include <cstring>
#include <memory>
#include <vector>

#include "../../include/ddlo_track.h"
#include "runtime.hpp"
#include "track_core.hpp"
#include "track_internal.hpp"

using ddlo::rt::fail;
namespace trk = ddlo::trk;

struct ddlo_track {
  trk::Tracker t;
  double dt = 0.1;   // ddlo_track_decide's step
  std::vector<trk::Detection> dets;
  std::vector<int32_t> ids;
};

namespace {

// Object from the detection's record (getObject, detection.cpp:766-781):
// the float state widened, entries 7..9 zero, avg_residuum narrowed to the
// float Object::avg_residuum is
gicp_status to_detections(const ddlo_seg_object* objs, size_t n, std::vector<trk::Detection>& out) {
  out.resize(n);
  for (size_t i = 0; i < n; ++i) {
    trk::Detection& d = out[i];
    d = trk::Detection();
    d.id = objs[i].id;
    d.num_points = objs[i].num_points;
    if (d.num_points <= 0) return fail(GICP_EINVAL, "a detection without points");
    for (int k = 0; k < 7; ++k) {
      if (!std::isfinite(objs[i].state[k])) return fail(GICP_EINVAL, "a detection with a non-finite state");
      d.state[k] = (double)objs[i].state[k];
    }
    d.avg_residuum = (float)objs[i].avg_residuum;
  }
  return GICP_OK;
}

void fill_result(const trk::Tracker& t, ddlo_track_result* r) {
  if (!r) return;
  std::memset(r, 0, sizeof(*r));
  r->undefined_tracks = (int32_t)t.count(DDLO_TRACK_MASK_UNDEFINED);
  r->static_tracks = (int32_t)t.count(DDLO_TRACK_MASK_STATIC);
  r->dynamic_tracks = (int32_t)t.count(DDLO_TRACK_MASK_DYNAMIC);
  r->matches = (int32_t)t.matches.size();
  r->created = (int32_t)t.unmatched_detections.size();
  r->erased = (int32_t)t.erased.size();
  r->turned_dynamic = t.turned_dynamic;
  r->boxes_cleared = t.boxes_collected;
}

}  // namespace

namespace ddlo {

void track_live(const ddlo_track* t, std::vector<int32_t>& ids, std::vector<int32_t>& status) {
  ids.clear();
  status.clear();
  for (const trk::Filter& f : t->t.filters) {
    ids.push_back(f.filter_id);
    status.push_back(f.obj.status);
  }
}

const std::vector<int>& track_erased(const ddlo_track* t) { return t->t.erased; }

}  // namespace ddlo

extern "C" {

gicp_status ddlo_track_default_params(ddlo_track_params* p) {
  if (!p) return fail(GICP_EINVAL, "null params");
  std::memset(p, 0, sizeof(*p));
  p->max_no_hits = 30;              // cfg/ddlo.yaml:224-233
  p->min_dynamic_hits = 5;
  p->max_undefined_hits = 1;
  p->max_obj_velocity = 15.f;
  p->min_dist_from_origin = 0.75;
  p->residuum_height_ratio = 0.3;
  return GICP_OK;
}

gicp_status ddlo_track_create(const ddlo_track_params* p, ddlo_track** out) {
  if (!out) return fail(GICP_EINVAL, "null out");
  *out = nullptr;
  ddlo_track_params q;
  if (p) q = *p;
  else ddlo_track_default_params(&q);
  if (q.max_no_hits < 0 || q.min_dynamic_hits < 0 || q.max_undefined_hits < 0 || !(q.max_obj_velocity >= 0.f) ||
      !std::isfinite(q.min_dist_from_origin) || !std::isfinite(q.residuum_height_ratio))
    return fail(GICP_EINVAL, "invalid tracker parameters");
  auto t = std::make_unique<ddlo_track>();
  t->t.p.max_no_hits = (size_t)q.max_no_hits;
  t->t.p.min_dynamic_hits = (size_t)q.min_dynamic_hits;
  t->t.p.max_undefined_hits = (size_t)q.max_undefined_hits;
  t->t.p.max_obj_velocity = q.max_obj_velocity;
  t->t.p.min_travel_dist = q.min_dist_from_origin;
  t->t.p.res_height_ratio = q.residuum_height_ratio;
  *out = t.release();
  return GICP_OK;
}

gicp_status ddlo_track_destroy(ddlo_track* t) {
  delete t;
  return GICP_OK;
}

gicp_status ddlo_track_update(ddlo_track* t, double dt, const ddlo_seg_object* objs, size_t n, int32_t* out_track_id,
                              ddlo_track_result* res) {
  if (!t || (!objs && n) || !std::isfinite(dt)) return fail(GICP_EINVAL, "invalid argument");
  if (gicp_status st = to_detections(objs, n, t->dets)) return st;
  t->t.update((float)dt, t->dets);   // update(float dt, ...): tracking.cpp:27
  if (out_track_id)
    for (size_t i = 0; i < n; ++i) out_track_id[i] = t->t.track_of_detection[i];
  fill_result(t->t, res);
  return GICP_OK;
}

gicp_status ddlo_track_tracks(const ddlo_track* t, ddlo_track_record* out, size_t cap, size_t* n) {
  if (!t || !n || (!out && cap)) return fail(GICP_EINVAL, "invalid argument");
  *n = t->t.filters.size();
  for (size_t i = 0; i < *n && i < cap; ++i) {
    const trk::Filter& f = t->t.filters[i];
    ddlo_track_record& r = out[i];
    std::memset(&r, 0, sizeof(r));
    r.id = f.filter_id;
    r.status = f.obj.status;
    r.hits = (int32_t)f.hits;
    r.sslu = (int32_t)f.sslu;
    for (int k = 0; k < 10; ++k) r.state[k] = f.kf.x[k];
    r.num_points = f.obj.num_points;
    r.object_id = f.obj.id;
    r.avg_residuum = f.obj.avg_residuum;
    r.dist_to_origin = f.dist_to_origin();
    r.history = (int32_t)f.static_bboxes.size();
  }
  return GICP_OK;
}

gicp_status ddlo_track_count(const ddlo_track* t, int status_mask, size_t* n) {
  if (!t || !n) return fail(GICP_EINVAL, "null argument");
  *n = t->t.count(status_mask);
  return GICP_OK;
}

gicp_status ddlo_track_erased(const ddlo_track* t, int32_t* ids, size_t cap, size_t* n) {
  if (!t || !n || (!ids && cap)) return fail(GICP_EINVAL, "invalid argument");
  *n = t->t.erased.size();
  for (size_t i = 0; i < *n && i < cap; ++i) ids[i] = t->t.erased[i];
  return GICP_OK;
}

gicp_status ddlo_track_take_cleared_boxes(ddlo_track* t, ddlo_map_box* out, size_t cap, size_t* n) {
  if (!t || !n || (!out && cap)) return fail(GICP_EINVAL, "invalid argument");
  *n = t->t.cleared.size();
  if (!out) return GICP_OK;
  if (cap < *n) return fail(GICP_EINVAL, "box capacity too small");
  for (size_t i = 0; i < *n; ++i) {
    const trk::Box& b = t->t.cleared[i];
    for (int k = 0; k < 3; ++k) {
      out[i].position[k] = b.position[k];
      out[i].dimensions[k] = b.dimensions[k];
    }
    out[i].orientation_z = b.orientation_z;
  }
  t->t.cleared.clear();
  return GICP_OK;
}

gicp_status ddlo_track_last_costs(const ddlo_track* t, double* cost, float* disp, int32_t* assignment, size_t cap,
                                  int32_t* rows, int32_t* cols) {
  if (!t) return fail(GICP_EINVAL, "null handle");
  const size_t ne = t->t.cost.size();
  if (rows) *rows = t->t.rows;
  if (cols) *cols = t->t.cols;
  if ((cost || disp) && cap < ne) return fail(GICP_EINVAL, "matrix capacity too small");
  if (assignment && cap < (size_t)t->t.rows) return fail(GICP_EINVAL, "assignment capacity too small");
  if (cost && ne) std::memcpy(cost, t->t.cost.data(), sizeof(double) * ne);
  if (disp && ne) std::memcpy(disp, t->t.disp.data(), sizeof(float) * ne);
  if (assignment)
    for (int i = 0; i < t->t.rows; ++i) assignment[i] = t->t.assignment[i];
  return GICP_OK;
}

gicp_status ddlo_track_assign(const double* cost, int rows, int cols, int32_t* assignment) {
  if (!cost || !assignment || rows < 1 || cols < 1 || (long)rows * cols > (1L << 24))
    return fail(GICP_EINVAL, "invalid argument");
  for (long i = 0; i < (long)rows * cols; ++i)
    if (cost[i] != cost[i]) return fail(GICP_EINVAL, "NaN cost");
  std::vector<int> a((size_t)rows);
  trk::hungarian(cost, rows, cols, a.data());
  for (int i = 0; i < rows; ++i) assignment[i] = a[i];
  return GICP_OK;
}

int ddlo_track_decide(void* user, const ddlo_seg_object* objs, size_t n, uint8_t* non_static) {
  ddlo_track* t = static_cast<ddlo_track*>(user);
  if (!t || (!objs && n) || (!non_static && n)) return 1;
  t->ids.assign(n, -1);
  if (ddlo_track_update(t, t->dt, objs, n, t->ids.data(), nullptr) != GICP_OK) return 1;
  for (size_t i = 0; i < n; ++i) {
    non_static[i] = 0;
    for (const trk::Filter& f : t->t.filters)
      if (f.filter_id == t->ids[i]) non_static[i] = f.obj.status != trk::STATIC;
  }
  return 0;
}

gicp_status ddlo_track_set_dt(ddlo_track* t, double dt) {
  if (!t || !std::isfinite(dt)) return fail(GICP_EINVAL, "invalid argument");
  t->dt = dt;
  return GICP_OK;
}

}  // extern "C"
