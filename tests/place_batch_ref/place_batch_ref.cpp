// The host-side plan of the grouped place query (include/qtr_place_batch_math.h) and the layout of its item
// (include/quatro_place_batch.h), compiled with the host compiler for tests/test_place_batch_cpu.py.
#include <cstddef>

#include "qtr_place_batch_math.h"
#include "quatro_place_batch.h"

extern "C" {
void place_batch_ref_layout(int* out) {
  out[0] = (int)sizeof(qtr_place_query_item);
  out[1] = (int)offsetof(qtr_place_query_item, kf);
  out[2] = (int)offsetof(qtr_place_query_item, desc);
  out[3] = (int)offsetof(qtr_place_query_item, from);
  out[4] = (int)offsetof(qtr_place_query_item, entry);
  out[5] = (int)offsetof(qtr_place_query_item, mem);
  out[6] = (int)offsetof(qtr_place_query_item, id_lo);
  out[7] = (int)offsetof(qtr_place_query_item, id_hi);
  out[8] = (int)sizeof(qtr_place_match);
  out[9] = QTR_PLACE_BATCH_MAX;
  out[10] = QTR_PLACE_BATCH_MAX_PAIRS;
  out[11] = QTR_PLACE_BATCH_DIST;
  out[12] = QTR_PLACE_BATCH_SHIFT;
  out[13] = QTR_PLACE_BATCH_QT_CAP;
  out[14] = QTR_PLACE_BATCH_LDS_BYTES;
  out[15] = QTR_PLACE_BATCH_GRID_X;
  out[16] = (long long)QTR_PLACE_BATCH_MAX_PAIRS == QTR_PLACE_BATCH_PAIR_CAP;
}
int place_batch_ref_stride(int R, int S) { return qtr_place_batch_stride(R, S); }
int place_batch_ref_qt(int stride) { return qtr_place_batch_qt(stride); }
void place_batch_ref_clamp(int id_lo, int id_hi, int size, int* lo_hi) {
  qtr_place_batch_clamp(id_lo, id_hi, size, lo_hi, lo_hi + 1);
}
void place_batch_ref_union(const int* lo, const int* hi, int Q, int* ulo_uhi) {
  qtr_place_batch_union(lo, hi, Q, ulo_uhi, ulo_uhi + 1);
}
int place_batch_ref_pairs_ok(int Q, int U) { return qtr_place_batch_pairs_ok(Q, U); }
long long place_batch_ref_slot(int q, int e, int ulo, int U) { return (long long)qtr_place_batch_slot(q, e, ulo, U); }
}
