/* quatro_place_batch.h - C ABI of the grouped place query, exported by quatro_amd/libquatro_ext.so.
 *
 * The two entry points below work on the handles, keyframes and place indexes of libquatro_hip.so
 * (include/quatro_hip.h); include/quatro_voxelmap.h says what the extension library is.  Both libraries must come from the
 * same build.  The host-side plan of a call is include/qtr_place_batch_math.h; the arithmetic is include/qtr_place_math.h's,
 * unchanged.
 *
 * What qtr_submit_batch_keyframes is to registration, this is to the search in front of it: Q queries against one index in
 * ONE chain of launches and ONE host wait.  Every entry of the union of the queries' ranges is filled into LDS once per
 * tile of queries and scored against all of them.  Query q IS the single call of its source, range and k: row q of `out`
 * with n_out[q] equals what the single call returns, field for field and bit for bit: qtr_place_query for a keyframe item,
 * qtr_place_query_desc for a descriptor item and, on that entry's QTR_PLACE_DESC, for an entry item.  A query whose clamped range is empty gets
 * n_out[q] = 0 and does not affect the others.  Records of row q beyond n_out[q] are left as they were.
 *
 * An item names its source by the first of kf, desc, from/entry that is set: a keyframe (described from its stored voxels,
 * read in place), a descriptor of num_rings * num_sectors floats in `mem`, or entry `entry` of `from` (NULL: the searched
 * index itself; another index must have the searched index's num_rings and num_sectors), read in place.
 *
 * Every argument is checked before anything is enqueued.  Q == 0 returns QTR_OK at once.  Q < 0 or above
 * QTR_PLACE_BATCH_MAX, k outside 1 .. QTR_PLACE_MAX_K, a NULL pointer (index, items, out, n_out), a descriptor item whose
 * mem is neither QTR_MEM_HOST nor QTR_MEM_DEVICE, an item with no source (no kf, no desc and entry < 0), an entry outside
 * its index, a keyframe or index of another handle and a `from` index of another shape are QTR_ERR_BAD_ARG; Q times the
 * length of the union range above QTR_PLACE_BATCH_MAX_PAIRS is QTR_ERR_CAPACITY; the message names the item.  After an
 * error every n_out[q] is 0, `out` is untouched and nothing ran.
 *
 * The call is complete on return and only READS the index: the threading rules are qtr_place_query's (any number of slots
 * may query one index at once; adds must not overlap a query).  It works in a batch arena of the slot's own (grown to a
 * call's need, freed with the handle), never in the slot's single-query scratch. */
#ifndef QUATRO_PLACE_BATCH_C_H
#define QUATRO_PLACE_BATCH_C_H

#include "quatro_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef QTR_EXT_API /* (libquatro_ext.so's exports: csrc/exports_ext.map lists them, csrc/exports.map does not) */
#define QTR_EXT_API QTR_API
#endif

#define QTR_PLACE_BATCH_MAX 1024            /* queries per call */
#define QTR_PLACE_BATCH_MAX_PAIRS (1 << 26) /* Q x (entries of the union range) per call */

/* what qtr_place_batch_fetch hands out for query `query` of the slot's last batch */
#define QTR_PLACE_BATCH_DIST 1  /* float[n_q]: min-over-shifts distance of every entry of the query's range */
#define QTR_PLACE_BATCH_SHIFT 2 /* int32[n_q]: its shift */

typedef struct qtr_place_query_item {
  const qtr_keyframe* kf;      /* non-NULL: descriptor of the keyframe's stored voxels, read in place; else */
  const float* desc;           /* non-NULL: num_rings*num_sectors floats in `mem`; else */
  const qtr_place_index* from; /* entry `entry` of this index (NULL = the searched index), read in place */
  int entry, mem;
  int id_lo, id_hi; /* this query's range, clamped to [0, size] like qtr_place_query's */
} qtr_place_query_item;

QTR_EXT_API int qtr_place_query_batch(qtr_handle* h, int slot, const qtr_place_index* index,
                                      const qtr_place_query_item* items, int Q, int k, qtr_place_match* out /* Q x k */,
                                      int* n_out /* Q */);
/* the slot's last batch: section `what` of query `query`, n_q = the length of its clamped range, in id order.  Copies
 * min(bytes, what there is) bytes to dst (may be NULL) and returns what there is; -1: a bad slot, query or `what`, or no
 * batch has run on the slot */
QTR_EXT_API long long qtr_place_batch_fetch(qtr_handle* h, int slot, int query, int what, void* dst, size_t bytes);

#ifdef __cplusplus
}
#endif
#endif /* QUATRO_PLACE_BATCH_C_H */
