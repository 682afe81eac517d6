// track_replay.cpp — the tracker core (csrc/track_core.hpp) on scripted
// sequences, as a program of its own: tests/test_track_san.py builds it with
// -fsanitize=address,undefined and runs it.  Host code only.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../dynamic_direct_lidar_odometry_amd/csrc/track_core.hpp"

namespace trk = ddlo::trk;

static unsigned long long g_state = 88172645463325252ULL;
static double rnd() {   // xorshift: the same script on every run
  g_state ^= g_state << 13;
  g_state ^= g_state >> 7;
  g_state ^= g_state << 17;
  return (double)(g_state >> 11) / 9007199254740992.0;
}

static trk::Detection det(int id, double x, double y, double dz, int n, float res) {
  trk::Detection d;
  d.id = id;
  d.num_points = n;
  const float s[7] = {(float)x, (float)y, 0.5f, (float)(0.3 * (rnd() - 0.5)), 0.6f, 0.8f, (float)dz};
  for (int i = 0; i < 7; ++i) d.state[i] = s[i];
  d.avg_residuum = res;
  return d;
}

static int fail(const char* what) {
  std::fprintf(stderr, "track_replay: %s\n", what);
  return 1;
}

int main() {
  // 1. the solver on every shape up to 12 x 12 with tied entries, zeros and a plateau
  for (int r = 1; r <= 12; ++r)
    for (int c = 1; c <= 12; ++c)
      for (int kind = 0; kind < 3; ++kind) {
        std::vector<double> m((size_t)r * c);
        for (double& v : m) v = kind == 0 ? (double)(int)(rnd() * 9) / 8.0 : kind == 1 ? 0.0 : 0.8 + 0.025 * (int)(rnd() * 5);
        std::vector<int> a((size_t)r);
        trk::hungarian(m.data(), r, c, a.data());
        int assigned = 0;
        std::vector<char> used((size_t)c, 0);
        for (int i = 0; i < r; ++i)
          if (a[i] >= 0) {
            if (a[i] >= c || used[a[i]]) return fail("assignment is no matching");
            used[a[i]] = 1;
            ++assigned;
          }
        if (assigned != (r < c ? r : c)) return fail("assignment is not complete");
      }
  // 2. the IoU on identical, disjoint, touching, flat and rotated boxes
  {
    const double a[7] = {0, 0, 0.5, 0.0, 1, 2, 1}, b[7] = {10, 0, 0.5, 0.2, 1, 2, 1}, c[7] = {1, 0, 0.5, 0.0, 1, 2, 1},
                 f[7] = {0, 0, 0.5, 0.0, 0, 0, 0}, g[7] = {0.2, 0.1, 0.6, 0.4, 1.5, 0.7, 2};
    const double v = trk::iou::obb_iou(a, a);
    if (!(v > 0.999 && v <= 1.0)) return fail("IoU of identical boxes");
    if (trk::iou::obb_iou(a, b) != 0.0) return fail("IoU of disjoint boxes");
    if (trk::iou::obb_iou(f, f) != 0.0) return fail("IoU of two flat boxes");
    const double t = trk::iou::obb_iou(a, c), w = trk::iou::obb_iou(a, g);
    if (!(t >= 0.0 && t <= 1.0 && w > 0.0 && w < 1.0)) return fail("IoU range");
  }
  // 3. scripted sequences: walkers, pauses, gaps, crowds and empty frames, small and large erase limits
  for (int run = 0; run < 24; ++run) {
    trk::Tracker t;
    t.p.max_no_hits = run % 3 == 0 ? 2 : (run % 3 == 1 ? 6 : 30);
    t.p.max_undefined_hits = run % 2 ? 1 : 4;
    t.p.min_dynamic_hits = 3;
    t.p.res_height_ratio = run % 4 ? 0.3 : 0.0;
    size_t boxes = 0;
    for (int f = 0; f < 60; ++f) {
      std::vector<trk::Detection> dets;
      const int n = (f % 11 == 0) ? 0 : (int)(rnd() * 13);
      for (int k = 0; k < n; ++k) {
        const bool walker = k % 3 == 0;
        dets.push_back(det(k + 1, 3.0 * k + (walker ? 0.3 * f : 0.0) + 0.02 * rnd(), (k % 2 ? 4.0 : -4.0) + 0.02 * rnd(),
                           k % 5 == 4 ? 0.0 : 1.0 + 0.1 * k, 20 + 40 * k + (int)(rnd() * 9), (float)(walker ? 0.8 : 0.05)));
      }
      t.update(f % 7 == 3 ? 0.05f : 0.1f, dets);
      if (t.track_of_detection.size() != dets.size()) return fail("track ids");
      for (int id : t.track_of_detection)
        if (id < 0 || id >= t.next_id) return fail("track id range");
      for (const trk::Filter& fl : t.filters) {
        if (fl.sslu >= t.p.max_no_hits) return fail("a filter past max_no_hits survived");
        if (fl.static_bboxes.size() > 5) return fail("history longer than five");
        for (int i = 0; i < trk::KN; ++i)
          if (!(fl.kf.x[i] == fl.kf.x[i])) return fail("NaN state");
      }
      boxes += (size_t)t.boxes_collected;
    }
    if (t.cleared.size() != boxes) return fail("cleared boxes are not the sum of the frames'");
  }
  std::printf("track replay: ok\n");
  return 0;
}
