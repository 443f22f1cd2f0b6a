// qtr_vmap_batch_math.h — the contract of the grouped map registration (include/quatro_voxelmap_batch.h,
// quatro_amd/csrc/voxelmap_batch.hip), on top of qtr_vmap_math.h.
//
// An item of a batch IS one qtr_voxel_map_register with that item's cloud and guess: the member tests, qtr_vmap_query,
// qtr_icp_vgicp_terms, the chunk sums in chunk order, qtr_icp_step and the stops are qtr_vmap_math.h's and
// qtr_icp_math.h's, unchanged.  No arithmetic is new and the loop is not restated: the reference of every item is the
// restatement of the single call (tests/vmap_restate.py, RefMap.register).
//
// What is new are two host-side helpers, static inline with a fixed association so that C, C++ and the Python restatement
// (quatro_amd/api.py: pose_hypotheses, best_hypothesis) agree bit for bit:
//
//   qtr_vmap_hypothesis  out = base . [Rz(yaw) | (dx, dy, 0)]: a pose `base` (16 row-major doubles, rows 0 - 2 read) turned
//                        about ITS z by yaw and moved by (dx, dy) in ITS xy plane.  c = cos(yaw) and s = sin(yaw) come from
//                        libm on the host; per row r with b = base[4 r ..]:
//                          out[4 r + 0] = b0 c + b1 s        out[4 r + 1] = b1 c - b0 s        out[4 r + 2] = b2
//                          out[4 r + 3] = (b0 dx + b1 dy) + b3
//                        and row 3 is (0 0 0 1).  With `base` the pose of a place-index entry (entry frame -> map frame) and
//                        yaw the match's yaw (query -> entry, include/quatro_hip.h) this is a guess that maps the query's
//                        frame into the map's; a small grid of (yaw, dx, dy) around it are the hypotheses of a relocalisation.
//   qtr_vmap_batch_best  the winner among B results: only items with status == QTR_OK and valid count; the largest n_corr
//                        wins, ties go to the smaller rmse, then to the smaller index; -1 when no item qualifies (B <= 0
//                        included).
#ifndef QTR_VMAP_BATCH_MATH_H
#define QTR_VMAP_BATCH_MATH_H

#include <math.h>

#include "qtr_vmap_math.h"
#include "quatro_hip.h"

static inline void qtr_vmap_hypothesis(const double base[16], double yaw, double dx, double dy, double out[16]) {
  const double c = cos(yaw), s = sin(yaw);
  int r;
  for (r = 0; r < 3; ++r) {
    const double b0 = base[4 * r + 0], b1 = base[4 * r + 1], b2 = base[4 * r + 2], b3 = base[4 * r + 3];
    out[4 * r + 0] = b0 * c + b1 * s;
    out[4 * r + 1] = b1 * c - b0 * s;
    out[4 * r + 2] = b2;
    out[4 * r + 3] = (b0 * dx + b1 * dy) + b3;
  }
  out[12] = 0.0;
  out[13] = 0.0;
  out[14] = 0.0;
  out[15] = 1.0;
}

static inline int qtr_vmap_batch_best(const qtr_icp_result* r, int B) {
  int best = -1, i;
  for (i = 0; i < B; ++i) {
    if (r[i].status != QTR_OK || !r[i].valid) continue;
    if (best < 0 || r[i].n_corr > r[best].n_corr || (r[i].n_corr == r[best].n_corr && r[i].rmse < r[best].rmse)) best = i;
  }
  return best;
}

#endif  // QTR_VMAP_BATCH_MATH_H
