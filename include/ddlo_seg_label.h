/*
 * ddlo_seg_label.h — the labelling mode of a ddlo_seg and the device
 * labelling over caller images.  Part of ddlo_segment.h, which includes it;
 * include that header.
 */
#ifndef DDLO_SEG_LABEL_H
#define DDLO_SEG_LABEL_H

#include "ddlo_segment.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Labelling mode of a handle.  HOST (the default) is the reference's
   breadth-first search on the host over the images read back.  DEVICE
   computes the same labels, segment count and counts on the device without
   the search order (connected components; only a prefix of each candidate
   component's push sequence is replayed, for max_z) and reads back one small
   record per scan; the getters fetch the images they need on demand.  Its
   avg_residuals are defined differently: the positive residuals of a
   segment's pixels without its seed (its first pixel in row-major order),
   summed in double in row-major order, over their count -- within
   (m + 1) 2^-24 (relative, m terms) of the reference's float sum in push
   order, and bit-identical from run to run.
   DEVICE needs 0 <= win_col0 and win_col1 <= cols - 1 (a window reaching
   outside the columns wraps, and the result then depends on the search
   order): otherwise ddlo_seg_set_labelling returns GICP_EINVAL and the mode
   is unchanged.  Changing the mode discards the last scan's results. */
#define DDLO_SEG_LABEL_HOST   0   /* default */
#define DDLO_SEG_LABEL_DEVICE 1
gicp_status ddlo_seg_set_labelling(ddlo_seg* s, int mode);
gicp_status ddlo_seg_get_labelling(const ddlo_seg* s, int* mode);

/* ddlo_seg_label on the device, over caller images (same arguments and
   in/out meaning); avg_residual per the device definition above. */
gicp_status ddlo_seg_label_device(int device, const ddlo_seg_params* p, const float* range, const float* z,
                                  const float* residual, float sensor_z, int32_t* label,
                                  double* avg_residual, size_t avg_cap, int32_t* segments);

/* Diagnostics of the last scan processed in DEVICE mode: the components whose
   push prefix was replayed, and the longest prefix (pushes).  Either may be NULL. */
gicp_status ddlo_seg_labelling_stats(const ddlo_seg* s, int32_t* replayed, int32_t* longest_prefix);

#ifdef __cplusplus
}
#endif

#endif /* DDLO_SEG_LABEL_H */
