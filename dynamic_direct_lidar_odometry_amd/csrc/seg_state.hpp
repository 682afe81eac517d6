// seg_state.hpp — the segmentation handle, for the files that make it up:
// segment.hip (the scan, the labelling, the objects, the static cloud) and
// its parts seg_tracks.hip, seg_classes.hip and seg_project.hip.  The
// odometry driver does not include this: it talks to the segmentation
// through seg_internal.hpp.
#pragma once
#include <hip/hip_runtime.h>

#include <memory>
#include <vector>

#include "../../include/ddlo_segment.h"
#include "runtime.hpp"
#include "seg_internal.hpp"
#include "seg_label.hpp"

namespace ddlo {

// The labelling's queues, kept across scans (a ddlo_seg keeps one): a fresh
// set per scan cost four zero-filled allocations of the image size.
struct LabelWork {
  std::vector<int> qy, qx, py, px, rows_hit;
  std::vector<char> line_flag;   // all zero between components
  // the feasible segments' pixels in the order the labelling pushed them, as CSR:
  // seg_pix[seg_off[l] .. seg_off[l + 1]) for l = 1 .. segments (seg_off[0] = seg_off[1] = 0)
  std::vector<int> seg_off, seg_pix;
};

// The parts are defined in their own files and made by their first use; the
// handle owns them (each file defines its operator()).
struct SegTracks;    // the tracks' pixel lists (seg_tracks.hip), made by the first ddlo_seg_tracks_sync
struct SegClasses;   // the per-pixel classes (seg_classes.hip), made by the first ddlo_seg_classify
struct SegProject;   // the projection of unorganized clouds (seg_project.hip), made by the first projected scan
struct SegPartFree {
  void operator()(SegTracks* t) const;
  void operator()(SegClasses* c) const;
  void operator()(SegProject* p) const;
};

}  // namespace ddlo

struct ddlo_seg {
  int device = 0;
  ddlo_seg_params p{};
  hipStream_t s = nullptr;
  // the scan as ddlo_seg_process saw it (x, y, z floats first, raw_stride
  // bytes apart; never the packed copy the static cloud writes NaN over) and its images
  ddlo::rt::DevBuf raw, range, ground, label;
  size_t raw_stride = 0;
  // objects and the static cloud: the segments' pixel lists and the object
  // records on the device; the packed scan, the removed pixels and the filter scratch
  ddlo::rt::DevBuf zimg, dcsr, dobj, ddrop, f4, f4b, keep, pos, vscratch, cubtmp;
  // ddlo_seg_set_voxel_order: the static cloud's voxel pass, and the scratch only the PCL order needs
  int voxel_order = 0;
  ddlo::rt::DevBuf voscratch;
  // ddlo_seg_set_downsampling: the row/column filter's keyframe pass between the removal and the
  // crop (seg_static_finish): the workgroups' removed counts and the pass's control words, and
  // whether the last pass met |S| > n' (read back with the filters' count, cnt_pin[16])
  int ds_use = 0, ds_row = 1, ds_col = 1;
  ddlo::rt::DevBuf ds_part;
  bool ds_skipped = false;
  // ddlo_seg_set_intensity: the static cloud's w is the channel, read from raw at inten_off (a scan of
  // ddlo_seg_process) or at 12 (raw_staged: the float4 scan the driver or the projection staged).  The
  // removal then cannot mark a pixel in w: with the row/column filter on it marks rm_flags instead.
  int inten_use = 0;
  size_t inten_off = 0, raw_inten_off = 0;   // raw_inten_off: what the scan in raw was uploaded with (0: x, y, z alone)
  bool raw_staged = false;
  ddlo::rt::DevBuf rm_flags;
  bool have_objects = false;         // objects holds the last scan's records
  std::vector<ddlo_seg_object> objects;   // every segment's record of the last scan (before the ratio test)
  // seg_csr: the last scan's segments are on the device (host labelling: dcsr
  // holds them) / their lengths are in csr_len.  Reset with every scan.
  bool csr_ready = false, csr_len_ready = false;
  std::vector<int> csr_len;
  ddlo::rt::PinBuf cnt_pin;           // the filters' count read-back
  ddlo::rt::PinBuf obj_stage;         // the object kernel's pixel lists in, records out
  ddlo::rt::PinBuf drop_stage;        // the removed segments' pixels
  ddlo::rt::PinBuf pin;               // range | label | z (staged scans) | ground
  std::vector<float> z;
  // the last scan's images: the pinned read-back buffers themselves (the
  // labelling rewrites h_label in place)
  const float* h_range = nullptr;
  const signed char* h_ground = nullptr;
  int* h_label = nullptr;
  size_t hn = 0;
  std::vector<double> avg;
  ddlo::LabelWork work;
  bool have = false;                  // a scan was processed: the fields above are its
  ddlo_seg_result last{};
  // device labelling (ddlo_seg_set_labelling): its scratch and results, the
  // residual image on the device, the pinned record read back per frame, and
  // which host images (kImg*) the getters have fetched for the last scan
  int labelling = DDLO_SEG_LABEL_HOST;
  ddlo::LabelDev ldev;
  ddlo::rt::DevBuf dresid, dids;
  ddlo::rt::PinBuf rec_pin;
  unsigned fetched = 0;
  int replayed = 0, longest_prefix = 0;
  // counts the scans handed in, so that a part's data is known to be of the last one
  unsigned long long scan_serial = 0;
  std::unique_ptr<ddlo::SegTracks, ddlo::SegPartFree> tracks;
  std::unique_ptr<ddlo::SegClasses, ddlo::SegPartFree> classes;
  std::unique_ptr<ddlo::SegProject, ddlo::SegPartFree> project;
};

namespace ddlo {

enum : unsigned { kImgRange = 1, kImgGround = 2, kImgLabel = 4 };
// device mode: the host images a getter needs, read back once per scan
gicp_status fetch_images(ddlo_seg* s, unsigned want);

// The last scan's segments as CSR on the device, in either labelling mode:
// segment l's pixels are d_pix[d_off[l] .. d_off[l + 1]), l = 1 .. L, and
// len[l] of them (len: L + 1 entries, the handle's, valid until the next
// scan).  Made once per scan by whoever asks first.  Host labelling: the
// upload is enqueued on s->s, not waited for.
struct SegCsr {
  int L = 0;
  const int* d_off = nullptr;
  const int* d_pix = nullptr;
  const int* len = nullptr;
};
gicp_status seg_csr(ddlo_seg* s, SegCsr* out);

// ddlo_seg_static_cloud* in three steps.  begin: the checks, the scratch, the
// scan packed into s->f4.  Then the caller's removal: (NaN, NaN, NaN,
// kRemovedW) over points of s->f4, on s->s; or, where seg_removed_flags(s) is
// not null (cleared by begin), NaN over x, y, z and 1 in the pixel's flag.  finish: the row/column filter's
// keyframe pass if it is on (ddlo_seg_set_downsampling), then the voxel filter
// or the crop box into *pts / *count (valid until the next call on s);
// complete when it returns.
gicp_status seg_static_begin(ddlo_seg* s, const float centre[3], const float4** pts, int* count);
gicp_status seg_static_finish(ddlo_seg* s, const float centre[3], double crop_size, double leaf, const float4** pts,
                              int* count);
// The byte per pixel that marks a removed pixel for the row/column filter's keyframe pass when w is the
// intensity and cannot; nullptr when the marker in w does (intensity off), or nobody reads it (filter off).
inline unsigned char* seg_removed_flags(const ddlo_seg* s) {
  return s->inten_use && s->ds_use ? s->rm_flags.as<unsigned char>() : nullptr;
}
// where the intensity of the scan in s->raw sits in its records; 0: not carried
inline size_t seg_raw_intensity_offset(const ddlo_seg* s) {
  return s->inten_use ? (s->raw_staged ? (size_t)12 : s->raw_inten_off) : 0;
}

}  // namespace ddlo
