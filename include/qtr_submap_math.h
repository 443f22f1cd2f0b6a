// qtr_submap_math.h — the arithmetic of the keyframe merge (qtr_keyframe_merge: keyframes fused into one submap keyframe under
// their poses), shared by the gfx950 kernel (quatro_amd/csrc/keyframe.hip, k_kf_gather) and any host restatement, in the
// style of qtr_place_math.h / qtr_icp_math.h.  Both sides compile with -ffp-contract=off: NO product-sum below is fused, so
// a plain binary64 restatement reproduces every bit.
//
// A pose T is 16 doubles, row-major; rows 0 - 2 are used, row 3 is ignored.  A stored voxel record (x, y, z, w) becomes
//   X = (float)(((T[0] * (double)x + T[1] * (double)y) + T[2]  * (double)z) + T[3])
//   Y = (float)(((T[4] * (double)x + T[5] * (double)y) + T[6]  * (double)z) + T[7])
//   Z = (float)(((T[8] * (double)x + T[9] * (double)y) + T[10] * (double)z) + T[11])
// in binary64, in exactly that association, rounded ONCE to binary32; w is copied as stored (its bits, whatever they are).
// An identity pose reproduces a finite record bit for bit: 1 * x is x, the products with 0 are zeros and adding a zero
// changes nothing — with the one exception IEEE addition makes for a coordinate that is -0.0, which comes back as +0.0.
#pragma once
#include "qtr_math.h"

#define QTR_SUBMAP_POSE_DOUBLES 16

// one coordinate: row = T + 4 * r
QM_HD float qtr_submap_coord(const double* row, float x, float y, float z) {
  return (float)(((row[0] * (double)x + row[1] * (double)y) + row[2] * (double)z) + row[3]);
}

// the three coordinates of one record under T
QM_HD void qtr_submap_point(const double* T, float x, float y, float z, float* X, float* Y, float* Z) {
  *X = qtr_submap_coord(T, x, y, z);
  *Y = qtr_submap_coord(T + 4, x, y, z);
  *Z = qtr_submap_coord(T + 8, x, y, z);
}

// rows 0 - 2 finite?  (a pose with a NaN or an infinity there is refused before anything is enqueued)
QM_HD int qtr_submap_pose_finite(const double* T) {
  for (int i = 0; i < 12; ++i)
    if ((T[i] - T[i]) != 0.0) return 0;
  return 1;
}
