/* quatro_voxelmap_eval.h - C ABI of a pose evaluated against the voxel map, without stepping it, exported by
 * quatro_amd/libquatro_ext.so.
 *
 * The five entry points below work on the handles and keyframes of libquatro_hip.so (include/quatro_hip.h) and the maps of
 * include/quatro_voxelmap.h, which says what the extension library is.  Both libraries must come from the same build.  The
 * contract is include/qtr_vmap_eval_math.h.
 *
 * What qtr_evaluate* is to a pair of clouds, this is to a scan and a map: how much of the scan lies in voxels of the map
 * under T (overlap), how far from their means (inlier_rmse), the registration's own cost at T (chi2, rmse), the 6x6
 * information matrix of the edge scan -> map in Open3D's form (rotation first, [5][5] = n_corr) and the registration's
 * normal matrix and gradient at T (hessian, gradient).  The matched set at T is exactly the set one iteration of
 * qtr_voxel_map_register from T linearises on; nothing is solved and T is not changed.  information goes into a pose-graph
 * edge as it is; the eigenvalues of hessian say whether the localisation is degenerate (a corridor, an open field).
 *
 * One call evaluates up to QTR_VMAP_EVAL_MAX items in ONE launch (blockIdx.y = item) between one upload of the views and
 * poses and one copy of the records: scoring a pose hypothesis costs one evaluation, not a registration.  Item i IS the
 * single call of its cloud and pose: results[i] equals it field for field and bit for bit.  An item with n == 0 gets the
 * empty record (valid 0, every sum 0).
 *
 * With prm->per_point != 0 (at most QTR_VMAP_BATCH_MAX items) every point also gets a label: corr = 0 matched / -1 not, and
 * (w d^T M d, w) of its match, (0, 0) otherwise.  A weight of 0 marks a point the map does not explain: new or moving
 * geometry a caller may want to drop before an insert.
 *
 * Every argument is checked before anything is enqueued.  B == 0 returns QTR_OK at once.  B < 0, B above the limit, a NULL
 * pointer (items, prm, results; an item's src4 with n > 0, its src_normals4), n < 0, a mem that is neither QTR_MEM_HOST
 * nor QTR_MEM_DEVICE, a map or keyframe of another handle and a pose with a non-finite entry in rows 0 - 2 are
 * QTR_ERR_BAD_ARG; n > max_points is QTR_ERR_CAPACITY; the message names the item.  After such an error every
 * results[i].status is QTR_ERR_NOT_RUN and nothing ran.
 *
 * The call is host-synchronous on the slot's stream and only READS the map: other slots may evaluate, register or batch
 * against the same map at the same time.  It works in an arena of the slot's own (allocated on the slot's first evaluation,
 * grown to a call's need, freed with the handle), never in the slot's ICP, pair-evaluation or batch arenas: qtr_debug_fetch
 * and qtr_voxel_map_batch_fetch still serve the slot's last calls of those kinds.  Host-resident clouds are copied once per
 * distinct (pointers, n); keyframes and device-resident clouds are read in place. */
#ifndef QUATRO_VOXELMAP_EVAL_C_H
#define QUATRO_VOXELMAP_EVAL_C_H

#include "quatro_voxelmap_batch.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef QTR_EXT_API /* (libquatro_ext.so's exports: csrc/exports_ext.map lists them, csrc/exports.map does not) */
#define QTR_EXT_API QTR_API
#endif

#define QTR_VMAP_EVAL_MAX 1024 /* items of one call without per-point output (with it: QTR_VMAP_BATCH_MAX) */

/* what qtr_voxel_map_eval_fetch hands out for item `item` of the slot's last evaluation */
#define QTR_VMAP_EVAL_CORR 1  /* int32[n]: 0 matched, -1 none (per_point calls only) */
#define QTR_VMAP_EVAL_POINT 2 /* double[n][2]: (w d^T M d, w) of a matched point, (0, 0) otherwise (per_point calls only) */
#define QTR_VMAP_EVAL_TIMES 3 /* float[1]: device ms of the upload and the launch (the whole call's; `item` is ignored) */

typedef struct qtr_vmap_eval_params {
  int per_point; /* != 0: keep CORR and POINT of every item */
  int reserved[3];
} qtr_vmap_eval_params;

typedef struct qtr_vmap_eval_result {
  int status; /* QTR_OK, or QTR_ERR_NOT_RUN after a refused call */
  int valid;  /* n_corr > 0 */
  int n_source, n_corr;
  double overlap;     /* n_corr / n_source */
  double sum_d2;      /* sum |T p - mu|^2 over the matched points */
  double inlier_rmse; /* sqrt(sum_d2 / n_corr) */
  double sum_w;       /* sum of the matched voxels' member counts */
  double chi2;        /* sum w d^T M d */
  double rmse;        /* sqrt(chi2 / sum_w): qtr_voxel_map_register's rmse at T */
  double information[36]; /* row-major, rotation first; on the voxel means (the map's frame) */
  double hessian[36];     /* sum w J^T M J at T */
  double gradient[6];     /* sum w J^T M d at T */
} qtr_vmap_eval_result;

QTR_EXT_API void qtr_default_vmap_eval_params(qtr_vmap_eval_params* prm);
QTR_EXT_API int qtr_voxel_map_evaluate(qtr_handle* h, int slot, const qtr_voxel_map* map, const float* src4,
                                       const float* src_normals4, int n, int mem, const double T[16],
                                       const qtr_vmap_eval_params* prm, qtr_vmap_eval_result* result);
QTR_EXT_API int qtr_voxel_map_evaluate_keyframe(qtr_handle* h, int slot, const qtr_voxel_map* map, const qtr_keyframe* kf,
                                                const double T[16], const qtr_vmap_eval_params* prm,
                                                qtr_vmap_eval_result* result);
/* items[i].guess is the pose of item i */
QTR_EXT_API int qtr_voxel_map_evaluate_batch(qtr_handle* h, int slot, const qtr_voxel_map* map,
                                             const qtr_vmap_reg_item* items, int B, const qtr_vmap_eval_params* prm,
                                             qtr_vmap_eval_result* results /* [B] */);
/* copies min(bytes, what there is) bytes to dst (may be NULL) and returns what there is; -1: a bad slot, item or `what`, no
 * evaluation has run on the slot, or a per-point section after a call that did not ask for it */
QTR_EXT_API long long qtr_voxel_map_eval_fetch(qtr_handle* h, int slot, int item, int what, void* dst, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* QUATRO_VOXELMAP_EVAL_C_H */
