/*
 * ddlo_seg_tracks.h — the tracks' pixel lists, kept on the device by the
 * segmentation handle.  Part of ddlo_segment.h, which includes it.
 *
 * The reference removes from every scan the union of `indices` of all
 * UNDEFINED or DYNAMIC filters (odom.cc:867-892, tracking.cpp:192-208), and a
 * filter that was not matched this frame still holds the pixel indices of the
 * scan it last matched (bounding_box_filter.cpp:69,133-136): those stale
 * pixels are cut out of later scans for up to maxNoHits frames.  The lists
 * therefore outlive their scan.  They live here because this handle owns the
 * scan buffer, the segments' pixel lists and the stream, and its image shape
 * is fixed: a pixel index of an older scan is a valid index of the current one.
 *
 * The pool is two int buffers that swap: ddlo_seg_tracks_sync gathers the
 * surviving lists and the newly set ones into the other buffer in one launch
 * (k_trk_gather; offsets are a host prefix sum, no atomics), which grows
 * geometrically when it is too small.  A call that sets and releases nothing
 * launches nothing.
 */
#ifndef DDLO_SEG_TRACKS_H
#define DDLO_SEG_TRACKS_H

#include "ddlo_segment.h"

#ifdef __cplusplus
extern "C" {
#endif

/* track_ids[i]'s list becomes the pixel list of segment seg_ids[i] of the
   last ddlo_seg_process (replacing the one it held); the tracks in dead_ids
   release theirs; every other track keeps its list.  A segment id outside
   1 .. segments, a track id named twice, or a dead id that holds no list is
   GICP_EINVAL and changes nothing. */
gicp_status ddlo_seg_tracks_sync(ddlo_seg* s, const int32_t* track_ids, const int32_t* seg_ids, size_t n_set,
                                 const int32_t* dead_ids, size_t n_dead);

/* ddlo_seg_static_cloud (ddlo_seg_objects.h) with the union of the lists of
   the tracks in track_ids removed from the last scan instead of segments:
   the same packing, crop box, voxel filter and order-keeping compaction.  A
   track id that holds no list is GICP_EINVAL. */
gicp_status ddlo_seg_static_cloud_tracks(ddlo_seg* s, const int32_t* track_ids, size_t n, const float centre[3],
                                         double crop_size, double leaf, float* out, size_t cap, size_t* nout);

/* The list of one track (getIndices of one filter), in the order
   ddlo_seg_label_indices gives a segment's pixels: ascending row-major index.
   out[i] for i < cap; *n = the list's length. */
gicp_status ddlo_seg_track_indices(ddlo_seg* s, int32_t track_id, int32_t* out, size_t cap, size_t* n);

/* Lists held, indices held, and the capacity (in indices) of the pool buffer in use. */
gicp_status ddlo_seg_tracks_stats(const ddlo_seg* s, int32_t* lists, int64_t* indices, int64_t* capacity);

#ifdef __cplusplus
}
#endif

#endif /* DDLO_SEG_TRACKS_H */
