// eval.cpp — the evaluation files of DetectionModule::evaluate
// (include/ddlo_eval.h).  Host code only.
#include <cerrno>
#include <cinttypes>
#include <cstdio>
#include <cstring>
#include <filesystem>
#include <string>
#include <system_error>

#include "../../include/ddlo_eval.h"
#include "runtime.hpp"

using ddlo::rt::fail;

struct ddlo_eval {
  std::string dir;
};

namespace {

// Eigen's default IOFormat on a 4 x 4 float matrix: every coefficient as an
// ostream prints a float at precision 6 (%.6g), right-aligned to the widest
std::string format_pose(const float T[16]) {
  char cell[16][32];
  int width = 0;
  for (int i = 0; i < 16; ++i) {
    const int w = std::snprintf(cell[i], sizeof(cell[i]), "%.6g", (double)T[i]);
    width = w > width ? w : width;
  }
  std::string s;
  for (int r = 0; r < 4; ++r) {
    if (r) s += '\n';
    for (int c = 0; c < 4; ++c) {
      if (c) s += ' ';
      const std::string v = cell[4 * r + c];
      s.append((size_t)width - v.size(), ' ');
      s += v;
    }
  }
  return s;
}

gicp_status io_fail(const std::string& what, const std::string& path) {
  return fail(GICP_EINVAL, what + " " + path + ": " + std::strerror(errno));
}

}  // namespace

extern "C" {

gicp_status ddlo_eval_open(const char* dir, ddlo_eval** out) {
  if (!dir || !*dir || !out) return fail(GICP_EINVAL, "invalid argument");
  *out = nullptr;
  std::error_code ec;
  std::filesystem::create_directories(dir, ec);
  if (ec || !std::filesystem::is_directory(dir, ec))
    return fail(GICP_EINVAL, std::string("cannot create the evaluation directory ") + dir + ": " + ec.message());
  // the pose file is opened for appending now: a directory that cannot be written fails here, not at the first frame
  const std::string poses = std::string(dir) + "/poses.txt";
  FILE* f = std::fopen(poses.c_str(), "a");
  if (!f) return io_fail("cannot open", poses);
  std::fclose(f);
  *out = new ddlo_eval{dir};
  return GICP_OK;
}

gicp_status ddlo_eval_write(ddlo_eval* e, uint32_t seq, uint64_t stamp_ns, const float T[16], const int32_t* dynamic_idx,
                            size_t n) {
  if (!e || !T || (n && !dynamic_idx)) return fail(GICP_EINVAL, "invalid argument");
  char name[32];
  std::snprintf(name, sizeof(name), "/%04u.txt", (unsigned)seq);
  const std::string idx_path = e->dir + name;
  FILE* f = std::fopen(idx_path.c_str(), "a");
  if (!f) return io_fail("cannot open", idx_path);
  bool ok = true;
  for (size_t i = 0; i < n && ok; ++i) ok = std::fprintf(f, "%d\n", (int)dynamic_idx[i]) > 0;
  ok = (std::fclose(f) == 0) && ok;
  if (!ok) return io_fail("cannot write", idx_path);
  const std::string poses = e->dir + "/poses.txt";
  f = std::fopen(poses.c_str(), "a");
  if (!f) return io_fail("cannot open", poses);
  ok = std::fprintf(f, "%" PRIu64 "\n%s;\n", stamp_ns, format_pose(T).c_str()) > 0;
  ok = (std::fclose(f) == 0) && ok;
  if (!ok) return io_fail("cannot write", poses);
  return GICP_OK;
}

gicp_status ddlo_eval_close(ddlo_eval* e) {
  delete e;
  return GICP_OK;
}

}  // extern "C"
