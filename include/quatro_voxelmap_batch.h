/* quatro_voxelmap_batch.h - C ABI of a batch of scans and guesses registered against one voxel map in one chain of
 * launches, exported by quatro_amd/libquatro_ext.so.
 *
 * The two entry points below work on the handles and keyframes of libquatro_hip.so (include/quatro_hip.h) and the maps of
 * include/quatro_voxelmap.h, which says what the extension library is.  Both libraries must come from the same build.  The
 * contract is include/qtr_vmap_batch_math.h.
 *
 * Plane-to-plane against voxels of side c captures about one voxel, so finding a scan's pose in a finished map without a
 * good guess means trying many guesses: the k candidates of a place query, each with a small grid of yaw and xy offsets
 * (qtr_vmap_hypothesis), a fleet of scans against one map, or a window of keyframes after a pose-graph optimisation.  One
 * call here takes up to QTR_VMAP_BATCH_MAX items.  Item i IS one single registration (of a cloud, or of a keyframe) with that
 * item's cloud and guess: results[i] equals, field for field and bit for bit, what the single call returns for it alone; an item
 * with n == 0 gets the empty result (the guess, no correspondence, QTR_ICP_STOP_TOO_FEW).  qtr_vmap_batch_best picks the
 * winner.
 *
 * One launch initialises every item's state, then max_iterations launches run one iteration of every item each
 * (blockIdx.y = item; an item that stopped stays frozen), then the states are read back once.  With QTR_ICP_BLOCK = n in the
 * environment the host reads the states back after every n launches and ends the loop once all items have stopped, as the
 * single call does.
 *
 * Every argument is checked before anything is enqueued.  B == 0 returns QTR_OK at once.  B < 0, B > QTR_VMAP_BATCH_MAX, a
 * NULL pointer (items, prm, results; an item's src4 with n > 0, its src_normals4), n < 0, a mem that is neither
 * QTR_MEM_HOST nor QTR_MEM_DEVICE, a method other than QTR_ICP_VOXEL_PLANE_TO_PLANE, a map or keyframe of another handle and
 * a guess with a non-finite entry in rows 0 - 2 are QTR_ERR_BAD_ARG; n > max_points is QTR_ERR_CAPACITY.  After such an
 * error every results[i].status is QTR_ERR_NOT_RUN and nothing ran.
 *
 * The call is host-synchronous on the slot's stream and only READS the map: other slots may register or batch against the
 * same map at the same time; inserts, clear, evict, restore and carve on that map are the caller's to serialise against it.
 * It works in a batch arena of the slot's own (allocated on the slot's first batch, grown to a call's need, freed with the
 * handle): per item one state, one ticket, its partial sums, its trace (max_iterations x 18 doubles) and its
 * correspondence flags (n ints), and a copy of every host-resident cloud.  Keyframes and device-resident clouds are read in
 * place.  The slot's single-call ICP state, and what qtr_debug_fetch serves for it, are left untouched. */
#ifndef QUATRO_VOXELMAP_BATCH_C_H
#define QUATRO_VOXELMAP_BATCH_C_H

#include "quatro_voxelmap.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef QTR_EXT_API /* (libquatro_ext.so's exports: csrc/exports_ext.map lists them, csrc/exports.map does not) */
#define QTR_EXT_API QTR_API
#endif

#define QTR_VMAP_BATCH_MAX 64

/* what qtr_voxel_map_batch_fetch hands out for item `item` of the slot's last batch: the per-item counterparts of
 * QTR_DBG_ICP_TRACE / _CORR / _TIMES */
#define QTR_VMAP_BATCH_TRACE 1 /* double[iterations][18]: one row per update */
#define QTR_VMAP_BATCH_CORR 2  /* int32[n]: 0 matched, -1 none, at the item's last evaluation */
#define QTR_VMAP_BATCH_TIMES 3 /* float[2]: device ms before the loop and of the loop (the whole batch's; `item` is ignored) */

typedef struct qtr_vmap_reg_item {
  const qtr_keyframe* kf;    /* non-NULL: the keyframe's voxels and normals, read in place; the next four are ignored */
  const float* src4;         /* else n records x,y,z,* ... */
  const float* src_normals4; /* ... and their normals (non-NULL) */
  int n, mem;                /* QTR_MEM_HOST / QTR_MEM_DEVICE */
  double guess[16];          /* rows 0 - 2 read, finite; row 3 taken as (0 0 0 1) */
} qtr_vmap_reg_item;

QTR_EXT_API int qtr_voxel_map_register_batch(qtr_handle* h, int slot, const qtr_voxel_map* map,
                                             const qtr_vmap_reg_item* items, int B, const qtr_icp_params* prm,
                                             qtr_icp_result* results /* [B] */);
/* copies min(bytes, what there is) bytes to dst (may be NULL) and returns what there is; -1: a bad slot, item or `what`, or
 * no batch has run on the slot */
QTR_EXT_API long long qtr_voxel_map_batch_fetch(qtr_handle* h, int slot, int item, int what, void* dst, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* QUATRO_VOXELMAP_BATCH_C_H */
