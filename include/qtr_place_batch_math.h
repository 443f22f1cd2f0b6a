// qtr_place_batch_math.h — the host-side plan of a grouped place query (include/quatro_place_batch.h,
// quatro_amd/csrc/place_batch.hip), in plain C.
//
// A query of a group IS one qtr_place_query / qtr_place_query_desc with that query's source, range and k: the cells, the
// column norms, d(s), the keys and the yaw are qtr_place_math.h's, unchanged.  No arithmetic is new.  What is new is how
// the host lays a call out, and the tests restate exactly that:
//
//   qtr_place_batch_clamp   a query's range [id_lo, id_hi) clamped to [0, size], as qtr_place_query does it:
//                           lo = max(id_lo, 0), hi = min(id_hi, size); empty (lo = hi = 0) unless hi > lo.
//   qtr_place_batch_union   the smallest [ulo, uhi) that holds every non-empty clamped range; (0, 0) when all are empty.
//                           Ranges may leave holes in it: a (query, entry) pair outside the query's range takes no part.
//   qtr_place_batch_qt      the query tile of k_place_score_group: the largest QT with (QT + 4) * stride * 4 <= 65536 bytes
//                           of LDS (QT queries and one entry per wave of the workgroup), at most QTR_PLACE_BATCH_QT_CAP.
//                           The largest legal entry (32 x 64: stride 2112 floats) would still leave 3, so QT >= 1 always.
//                           The cap is 2 because the score is bound by its LDS reads, not by the fill: a larger tile
//                           takes the LDS that further workgroups of a compute unit would need.
//   qtr_place_batch_pairs_ok  Q * (uhi - ulo) <= QTR_PLACE_BATCH_MAX_PAIRS, in 64-bit.
//   qtr_place_batch_slot    the score table is Q rows of U = uhi - ulo slots; (query q, entry e) is slot q * U + (e - ulo).
//                           A slot holds the single path's key, (distance bits << 32) | e, and — in a second array of the
//                           same shape — its shift; a pair outside the query's range holds the key ~0.
//   QTR_PLACE_BATCH_GRID_X  the widest grid.x of k_place_score_group: one pass covers 4 * QTR_PLACE_BATCH_GRID_X entries,
//                           a longer union range takes further rounds of the same workgroups.
#ifndef QTR_PLACE_BATCH_MATH_H
#define QTR_PLACE_BATCH_MATH_H

#include <stddef.h>

#if defined(__HIPCC__) /* the kernels call qtr_place_batch_slot */
#define QTR_PB_HD __host__ __device__ static inline
#else
#define QTR_PB_HD static inline
#endif

#define QTR_PLACE_BATCH_QT_CAP 2
#define QTR_PLACE_BATCH_LDS_BYTES 65536
#define QTR_PLACE_BATCH_GRID_X 2048
#define QTR_PLACE_BATCH_PAIR_CAP (1LL << 26) /* = QTR_PLACE_BATCH_MAX_PAIRS of include/quatro_place_batch.h */

static inline int qtr_place_batch_stride(int R, int S) { return ((R + 1) * S + 3) & ~3; }

static inline void qtr_place_batch_clamp(int id_lo, int id_hi, int size, int* lo, int* hi) {
  const int a = id_lo > 0 ? id_lo : 0, b = id_hi < size ? id_hi : size;
  if (b > a) {
    *lo = a;
    *hi = b;
  } else {
    *lo = 0;
    *hi = 0;
  }
}

/* lo / hi: Q clamped ranges */
static inline void qtr_place_batch_union(const int* lo, const int* hi, int Q, int* ulo, int* uhi) {
  int a = 0, b = 0, q;
  for (q = 0; q < Q; ++q) {
    if (!(hi[q] > lo[q])) continue;
    if (b == a) {
      a = lo[q];
      b = hi[q];
    } else {
      if (lo[q] < a) a = lo[q];
      if (hi[q] > b) b = hi[q];
    }
  }
  *ulo = a;
  *uhi = b;
}

static inline int qtr_place_batch_qt(int stride) {
  int qt = QTR_PLACE_BATCH_LDS_BYTES / (stride * 4) - 4;
  if (qt > QTR_PLACE_BATCH_QT_CAP) qt = QTR_PLACE_BATCH_QT_CAP;
  return qt;
}

static inline int qtr_place_batch_pairs_ok(int Q, int U) { return (long long)Q * (long long)U <= QTR_PLACE_BATCH_PAIR_CAP; }

QTR_PB_HD size_t qtr_place_batch_slot(int q, int e, int ulo, int U) { return (size_t)q * (size_t)U + (size_t)(e - ulo); }

#endif /* QTR_PLACE_BATCH_MATH_H */
