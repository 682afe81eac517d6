/*
 * ddlo_seg_objects.h — the detection half of the segmentation C-ABI: detected
 * objects and the scan without its non-static objects.  Part of
 * ddlo_segment.h, which includes it (and describes the calls and the
 * eigenvector convention of the boxes in its head comment).
 */
#ifndef DDLO_SEG_OBJECTS_H
#define DDLO_SEG_OBJECTS_H

#include "ddlo_segment.h"

#ifdef __cplusplus
extern "C" {
#endif

/* One detected object (the fields of Object, detection.h, that getObject and
   computeAllObjects fill). */
typedef struct ddlo_seg_object {
  int32_t id;            /* segment label, 1..segments */
  int32_t num_points;
  float   state[7];      /* x, y, z, sin(orientation/2), dx, dy, dz  (Object::state) */
  float   axis[2];       /* eigen_vectors_PCA.col(0): the minor principal axis in x-y (convention above) */
  float   density;       /* num_points / (dx*dy*dz); inf for a flat box */
  double  avg_residuum;  /* avg_residuals_[id], bit for bit */
} ddlo_seg_object;

/* Objects of the last ddlo_seg_process, ascending id, after the bounding-box
   ratio test (largest / second largest dimension >= max_dim_ratio drops the
   object, detection.cpp:800-804, in double on the float dimensions: 0 / 0 is
   NaN and passes, x / 0 is inf and is dropped; the code default is 10.0).
   Sums run in double in a fixed order: the result is the same bits from call
   to call.  state[2] and state[6] are the float 0.5f * (zmax + zmin) and
   zmax - zmin; the other fields are rounded once from double.  out[i] for
   i < cap; *n = number of objects (it may exceed cap). */
gicp_status ddlo_seg_objects(ddlo_seg* s, float max_dim_ratio, ddlo_seg_object* out, size_t cap, size_t* n);

/* The same over caller images (as ddlo_seg_label does for the labelling):
   world-frame points rows x cols (consecutive points stride_bytes apart), a
   label image (values <= 0 and DDLO_SEG_REJECTED are no segments; a label
   without pixels gives no object), avg_residual[l] for l < avg_n (NULL or
   l >= avg_n: 0). */
gicp_status ddlo_seg_objects_from(int device, const float* xyz_t, size_t stride_bytes, int rows, int cols,
                                  const int32_t* label, const double* avg_residual, size_t avg_n,
                                  float max_dim_ratio, ddlo_seg_object* out, size_t cap, size_t* n);

/* segmentation_scan_t_ after ExtractIndices(negative) of the pixels of the
   segments in remove_ids (each in 1 .. segments, else GICP_EINVAL), then
   CropBox(negative, [-crop_size, crop_size]^3 translated to centre,
   odom.cc:907-913; crop_size <= 0: off), then VoxelGrid(leaf) in the world
   frame (:914-918; leaf <= 0: off).  Non-finite pixels are always dropped
   (CropBox and VoxelGrid both skip them).  Input order is kept by the removal
   and the crop.  out: x, y, z float, 12 B each, cap points (more needed:
   GICP_EINVAL, *nout = the count); out may be NULL to query *nout. */
gicp_status ddlo_seg_static_cloud(ddlo_seg* s, const int32_t* remove_ids, size_t n_remove, const float centre[3],
                                  double crop_size, double leaf, float* out, size_t cap, size_t* nout);

#ifdef __cplusplus
}
#endif

#endif /* DDLO_SEG_OBJECTS_H */
