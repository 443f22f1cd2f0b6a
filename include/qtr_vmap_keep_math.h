// qtr_vmap_keep_math.h — the contract of the voxel map's upkeep (sliding-window eviction and restore), shared by the gfx950
// kernels (quatro_amd/csrc/voxelmap_keep.hip) and the host restatement of the tests (g++), on top of qtr_vmap_math.h, which
// stays as it is.  Integers decide everything here: no floating-point comparison settles a voxel's fate.
//
//   window   centre c[3] in metres, radius >= 0, on a grid of side s:  C_k = floor(c_k / s) as a double, a valid voxel
//            coordinate (-2^20 <= C_k < 2^20: qtr_vmap_coord, so NaN and infinities fail);  R = floor(radius / s) as a
//            double, < 2^22.  A negative or non-finite radius, or a centre outside the grid, is refused (false).
//   kept     a voxel with coordinates i is kept iff  sum_k (i_k - C_k)^2 <= R^2  in int64: |i_k - C_k| < 2^21, so the sum
//            is < 3 x 2^42 and R^2 < 2^44, both exact.
//   evict    the map afterwards is the map before without the voxels the rule rejects: count, acc[9] and the finished
//            record of a kept voxel are MOVED, never recomputed, so a later insert continues its acc as if nothing had
//            happened; an evicted voxel that is touched again starts from 0.0.
//   restore  n voxels as coords[n][3], count[n], sums[n][9] (the fetch sections COORDS, COUNT, SUMS) into a map that holds
//            no voxel: every coordinate valid, every count > 0, no coordinate triple twice.  The stored record is
//            qtr_icp_voxel_finish(sums, count, 0, .), as an insert's fold stores it.
#pragma once
#include "qtr_vmap_math.h"

#define QTR_VMAP_KEEP_RMAX 4194304.0  // 2^22: the window's radius in voxels stays below it

typedef struct QtrVmapWindow {
  int C[3];      // the centre's voxel
  long long R2;  // R^2, R = floor(radius / side) < 2^22
} QtrVmapWindow;

// the window of (centre, radius) on a grid of side c; false: refused
QM_HD bool qtr_vmap_window(const double* centre, double radius, double c, QtrVmapWindow* w) {
  if (!qtr_vmap_finite(radius) || !(radius >= 0.0)) return false;
  for (int a = 0; a < 3; ++a)
    if (!qtr_vmap_coord(centre[a], c, &w->C[a])) return false;
  const double R = floor(radius / c);
  if (!(R >= 0.0 && R < QTR_VMAP_KEEP_RMAX)) return false;
  const long long r = (long long)R;
  w->R2 = r * r;
  return true;
}

// the verdict on the voxel with coordinates i[3] (each in [-2^20, 2^20))
QM_HD bool qtr_vmap_kept(const QtrVmapWindow* w, const int* i) {
  long long s = 0;
  for (int a = 0; a < 3; ++a) {
    const long long d = (long long)i[a] - (long long)w->C[a];
    s = s + d * d;
  }
  return s <= w->R2;
}

QM_HD bool qtr_vmap_kept_key(const QtrVmapWindow* w, unsigned long long key) {
  int i[3];
  qtr_vmap_key_coords(key, i);
  return qtr_vmap_kept(w, i);
}

#define QTR_VMAP_RESTORE_OK 0
#define QTR_VMAP_RESTORE_BAD_COORD 1  // a coordinate outside [-2^20, 2^20)
#define QTR_VMAP_RESTORE_BAD_COUNT 2  // count <= 0

// one restored voxel: QTR_VMAP_RESTORE_OK and its key, or why it is refused (the coordinates are judged first)
QM_HD int qtr_vmap_restore_key(const int* i, int count, unsigned long long* key) {
  for (int a = 0; a < 3; ++a)
    if (i[a] < -1048576 || i[a] >= 1048576) return QTR_VMAP_RESTORE_BAD_COORD;
  if (count <= 0) return QTR_VMAP_RESTORE_BAD_COUNT;
  *key = qtr_vmap_key(i[0], i[1], i[2]);
  return QTR_VMAP_RESTORE_OK;
}
