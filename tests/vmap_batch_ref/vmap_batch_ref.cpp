// vmap_batch_ref.cpp — the two host-side helpers of include/qtr_vmap_batch_math.h behind a C interface, compiled by the tests
// with g++ -ffp-contract=off and held against their Python restatement (quatro_amd/api.py) bit for bit; and the layout of the
// batch item, for the ctypes mirror.
#include <cstddef>

#include "qtr_vmap_batch_math.h"
#include "quatro_voxelmap_batch.h"

extern "C" {
void vmap_batch_ref_hypothesis(const double* base, double yaw, double dx, double dy, double* out) {
  qtr_vmap_hypothesis(base, yaw, dx, dy, out);
}
int vmap_batch_ref_best(const qtr_icp_result* r, int B) { return qtr_vmap_batch_best(r, B); }
// sizeof(qtr_icp_result), sizeof(qtr_vmap_reg_item), the item's six offsets, QTR_VMAP_BATCH_MAX and the three fetch ids
void vmap_batch_ref_layout(int* out) {
  out[0] = (int)sizeof(qtr_icp_result);
  out[1] = (int)sizeof(qtr_vmap_reg_item);
  out[2] = (int)offsetof(qtr_vmap_reg_item, kf);
  out[3] = (int)offsetof(qtr_vmap_reg_item, src4);
  out[4] = (int)offsetof(qtr_vmap_reg_item, src_normals4);
  out[5] = (int)offsetof(qtr_vmap_reg_item, n);
  out[6] = (int)offsetof(qtr_vmap_reg_item, mem);
  out[7] = (int)offsetof(qtr_vmap_reg_item, guess);
  out[8] = QTR_VMAP_BATCH_MAX;
  out[9] = QTR_VMAP_BATCH_TRACE;
  out[10] = QTR_VMAP_BATCH_CORR;
  out[11] = QTR_VMAP_BATCH_TIMES;
}
}
