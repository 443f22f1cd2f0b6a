// quatro_voxelmap_batch.hpp — a batch of scans and guesses registered against a quatro_hip::VoxelMap (quatro_voxelmap.hpp) in
// one chain of launches, and the two helpers of a relocalisation, as free functions over qtr_voxel_map_register_batch,
// qtr_vmap_hypothesis and qtr_vmap_batch_best.  The calls are the extension library's
// (include/quatro_voxelmap_batch.h): link with -lquatro_hip -lquatro_ext.  Host code only.
#ifndef QUATRO_VOXELMAP_BATCH_H
#define QUATRO_VOXELMAP_BATCH_H

#include <algorithm>
#include <array>

#include "qtr_vmap_batch_math.h"
#include "quatro_voxelmap.hpp"
#include "quatro_voxelmap_batch.h"

namespace quatro_hip {

// an item: a keyframe's stored voxels and normals, read in place, under a guess (16 row-major doubles; nullptr = identity)
inline qtr_vmap_reg_item batch_item(const Keyframe& kf, const double* guess = nullptr) {
  qtr_vmap_reg_item it{};
  it.kf = kf.get();
  for (int k = 0; k < 16; ++k) it.guess[k] = guess ? guess[k] : (k % 5 == 0 ? 1.0 : 0.0);
  return it;
}

// an item: n records of 16 bytes in host memory with their normals
inline qtr_vmap_reg_item batch_item(const float* src4, const float* src_normals4, int n, const double* guess = nullptr) {
  qtr_vmap_reg_item it{};
  it.src4 = src4;
  it.src_normals4 = src_normals4;
  it.n = n;
  it.mem = QTR_MEM_HOST;
  for (int k = 0; k < 16; ++k) it.guess[k] = guess ? guess[k] : (k % 5 == 0 ? 1.0 : 0.0);
  return it;
}

// One result per item, each what VoxelMap::register_cloud / register_keyframe returns for that item alone, bit for bit.
// More than QTR_VMAP_BATCH_MAX items run in chunks of QTR_VMAP_BATCH_MAX in order.  The map is only read.
inline std::vector<qtr_icp_result> register_batch(const VoxelMap& map, const std::vector<qtr_vmap_reg_item>& items,
                                                  const qtr_icp_params& prm = default_map_icp_params()) {
  std::vector<qtr_icp_result> out(items.size());
  SlotLease lease;
  for (size_t at = 0; at < items.size(); at += QTR_VMAP_BATCH_MAX) {
    const int B = static_cast<int>(std::min<size_t>(QTR_VMAP_BATCH_MAX, items.size() - at));
    check(default_handle(),
          qtr_voxel_map_register_batch(default_handle(), lease.slot, map.get(), items.data() + at, B, &prm, out.data() + at));
  }
  return out;
}

// base . [Rz(yaw) | (dx, dy, 0)] (qtr_vmap_hypothesis): a guess around a pose
inline std::array<double, 16> hypothesis(const double* base, double yaw, double dx = 0.0, double dy = 0.0) {
  std::array<double, 16> out{};
  qtr_vmap_hypothesis(base, yaw, dx, dy, out.data());
  return out;
}

// the winner among the results (qtr_vmap_batch_best): the largest n_corr among the valid ones, then the smaller rmse, then
// the smaller index; -1 when none is valid
inline int best(const std::vector<qtr_icp_result>& results) {
  return qtr_vmap_batch_best(results.data(), static_cast<int>(results.size()));
}

}  // namespace quatro_hip
#endif  // QUATRO_VOXELMAP_BATCH_H
