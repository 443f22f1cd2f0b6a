// quatro_voxelmap_carve.hpp — visibility carving of a quatro_hip::VoxelMap (quatro_voxelmap.hpp): voxels that later scans see
// through leave the map, as free functions over qtr_voxel_map_carve / qtr_voxel_map_carve_keyframes.  The calls are
// the extension library's (include/quatro_voxelmap_carve.h): link with -lquatro_hip -lquatro_ext.  Host code only.
#ifndef QUATRO_VOXELMAP_CARVE_H
#define QUATRO_VOXELMAP_CARVE_H

#include "quatro_voxelmap.hpp"
#include "quatro_voxelmap_carve.h"

namespace quatro_hip {

inline qtr_carve_params default_carve_params() {
  qtr_carve_params p;
  qtr_default_carve_params(&p);
  return p;
}

// One scan (n records of 16 bytes in host memory, the RAW sweep rather than a ground-removed cloud) taken at pose (16
// row-major doubles, scan frame -> map frame; nullptr = identity): the voxels it saw through leave the map, the others stay
// bit for bit.  The caller serialises it against inserts, clear, evict and registrations on the map.
inline qtr_voxel_map_carve_info carve(VoxelMap& map, const float* xyz4, int n, const double* pose = nullptr,
                                      const qtr_carve_params& prm = default_carve_params()) {
  SlotLease lease;
  qtr_voxel_map_carve_info i{};
  check(default_handle(), qtr_voxel_map_carve(default_handle(), lease.slot, const_cast<qtr_voxel_map*>(map.get()), xyz4, n, pose, &prm,
                                              QTR_MEM_HOST, &i));
  return i;
}

// 1 .. 64 keyframes (never merged ones: they have no single viewpoint), each under its pose (16 doubles per keyframe); a
// voxel leaves when at least prm.min_votes of them saw through it
inline qtr_voxel_map_carve_info carve_keyframes(VoxelMap& map, const std::vector<const Keyframe*>& keyframes,
                                                const std::vector<double>& poses, const qtr_carve_params& prm = default_carve_params()) {
  if (poses.size() != 16 * keyframes.size()) throw std::invalid_argument("[quatro_hip] carve_keyframes: 16 doubles per keyframe");
  std::vector<const qtr_keyframe*> kfs;
  for (const Keyframe* k : keyframes) kfs.push_back(k ? k->get() : nullptr);
  SlotLease lease;
  qtr_voxel_map_carve_info i{};
  check(default_handle(), qtr_voxel_map_carve_keyframes(default_handle(), lease.slot, const_cast<qtr_voxel_map*>(map.get()), kfs.data(),
                                                        poses.data(), static_cast<int>(kfs.size()), &prm, &i));
  return i;
}

}  // namespace quatro_hip
#endif  // QUATRO_VOXELMAP_CARVE_H
