// quatro_voxelmap_eval.hpp — poses evaluated against a quatro_hip::VoxelMap (quatro_voxelmap.hpp) without stepping them, as
// free functions over qtr_voxel_map_evaluate, qtr_voxel_map_evaluate_batch and qtr_vmap_eval_best.  The items are
// quatro_voxelmap_batch.hpp's (batch_item; the guess is the pose).  The calls are the extension library's
// (include/quatro_voxelmap_eval.h): link with -lquatro_hip -lquatro_ext.  Host code only.
#ifndef QUATRO_VOXELMAP_EVAL_H
#define QUATRO_VOXELMAP_EVAL_H

#include <algorithm>
#include <vector>

#include "qtr_vmap_eval_math.h"
#include "quatro_voxelmap_batch.hpp"
#include "quatro_voxelmap_eval.h"

namespace quatro_hip {

// the scan (n records of 16 bytes in host memory with their normals) under the pose T (16 row-major doubles) against the map
inline qtr_vmap_eval_result evaluate(const VoxelMap& map, const float* src4, const float* src_normals4, int n, const double* T,
                                     bool per_point = false) {
  qtr_vmap_eval_params prm;
  qtr_default_vmap_eval_params(&prm);
  prm.per_point = per_point ? 1 : 0;
  qtr_vmap_eval_result res{};
  SlotLease lease;
  check(default_handle(),
        qtr_voxel_map_evaluate(default_handle(), lease.slot, map.get(), src4, src_normals4, n, QTR_MEM_HOST, T, &prm, &res));
  return res;
}

// One result per item, each what evaluate returns for that item alone, bit for bit; one launch per QTR_VMAP_EVAL_MAX items,
// in order.  The map is only read.
inline std::vector<qtr_vmap_eval_result> evaluate_batch(const VoxelMap& map, const std::vector<qtr_vmap_reg_item>& items) {
  qtr_vmap_eval_params prm;
  qtr_default_vmap_eval_params(&prm);
  std::vector<qtr_vmap_eval_result> out(items.size());
  SlotLease lease;
  for (size_t at = 0; at < items.size(); at += QTR_VMAP_EVAL_MAX) {
    const int B = static_cast<int>(std::min<size_t>(QTR_VMAP_EVAL_MAX, items.size() - at));
    check(default_handle(),
          qtr_voxel_map_evaluate_batch(default_handle(), lease.slot, map.get(), items.data() + at, B, &prm, out.data() + at));
  }
  return out;
}

// the winner among the evaluations (qtr_vmap_eval_best): the largest n_corr among the valid ones with status QTR_OK, then
// the smaller rmse, then the smaller index; -1 when none qualifies
inline int best(const std::vector<qtr_vmap_eval_result>& results) {
  std::vector<QtrVmapEvalRecord> rec(results.size());
  for (size_t i = 0; i < results.size(); ++i) {
    rec[i] = QtrVmapEvalRecord{};
    rec[i].valid = results[i].status == QTR_OK ? results[i].valid : 0;
    rec[i].n_corr = results[i].n_corr;
    rec[i].rmse = results[i].rmse;
  }
  return qtr_vmap_eval_best(rec.data(), static_cast<int>(rec.size()));
}

}  // namespace quatro_hip
#endif  // QUATRO_VOXELMAP_EVAL_H
