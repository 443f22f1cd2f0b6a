// quatro_voxelmap_keep.hpp — upkeep of a quatro_hip::VoxelMap (quatro_voxelmap.hpp): sliding-window eviction and restore
// from fetched sections, as free functions over qtr_voxel_map_evict / qtr_voxel_map_restore.  The two calls
// are the extension library's (include/quatro_voxelmap_keep.h): link with -lquatro_hip -lquatro_ext.  Host code only.
#ifndef QUATRO_VOXELMAP_KEEP_H
#define QUATRO_VOXELMAP_KEEP_H

#include "quatro_voxelmap.hpp"
#include "quatro_voxelmap_keep.h"

namespace quatro_hip {

// The voxels farther than floor(radius / voxel_size) voxels from the voxel of centre (3 doubles, metres) leave the map; the
// others stay bit for bit.  The caller serialises it against inserts, clear and registrations on the map.
inline qtr_voxel_map_evict_info evict(VoxelMap& map, const double* centre, double radius) {
  SlotLease lease;
  qtr_voxel_map_evict_info i{};
  check(default_handle(), qtr_voxel_map_evict(default_handle(), lease.slot, const_cast<qtr_voxel_map*>(map.get()), centre, radius, &i));
  return i;
}

// n voxels as the fetch sections QTR_VMAP_COORDS (3 n ints), QTR_VMAP_COUNT (n ints) and QTR_VMAP_SUMS (9 n doubles) in host
// memory, into a map that holds no voxel
inline void restore(VoxelMap& map, const std::vector<int>& coords, const std::vector<int>& count, const std::vector<double>& sums) {
  const size_t n = count.size();
  if (coords.size() != 3 * n || sums.size() != 9 * n) throw std::invalid_argument("[quatro_hip] restore: 3 coordinates and 9 sums per count");
  SlotLease lease;
  check(default_handle(), qtr_voxel_map_restore(default_handle(), lease.slot, const_cast<qtr_voxel_map*>(map.get()), coords.data(),
                                                count.data(), sums.data(), static_cast<int>(n), QTR_MEM_HOST));
}

// a copy of `map` with another capacity: restore of its three fetched sections
inline VoxelMap copy_map(const VoxelMap& map, int capacity) {
  VoxelMap out(map.info().voxel_size, capacity);
  restore(out, map.fetch<int>(QTR_VMAP_COORDS), map.fetch<int>(QTR_VMAP_COUNT), map.fetch<double>(QTR_VMAP_SUMS));
  return out;
}

}  // namespace quatro_hip
#endif  // QUATRO_VOXELMAP_KEEP_H
