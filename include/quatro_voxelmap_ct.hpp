// quatro_voxelmap_ct.hpp — the continuous-time registration of a raw sweep over quatro_voxelmap.hpp: the sensor's pose at the
// end of the sweep is fitted against the map while its pose at the beginning stays fixed, every point carried by the pose
// interpolated at its own time (include/quatro_voxelmap_ct.h).  Poses are 16 row-major doubles.
// Host code only; link with -lquatro_hip -lquatro_ext.
#ifndef QUATRO_VOXELMAP_CT_H
#define QUATRO_VOXELMAP_CT_H

#include <array>
#include <stdexcept>

#include "quatro_voxelmap.hpp"
#include "quatro_voxelmap_ct.h"

namespace quatro_hip {

// src4 / src_normals4: n records of 16 bytes, times: n floats, all in host memory; guess_end nullptr: begin_pose.
// The result's T is the end pose; info (may be nullptr) receives the counts of skipped and extrapolated points.
inline qtr_icp_result register_ct(const VoxelMap& map, const float* src4, const float* src_normals4, const float* times, int n,
                                  double t_begin, double t_end, const double* begin_pose, const double* guess_end = nullptr,
                                  const qtr_icp_params& prm = default_map_icp_params(), qtr_vmap_ct_info* info = nullptr) {
  SlotLease lease;
  qtr_icp_result r{};
  check(default_handle(), qtr_voxel_map_register_ct(default_handle(), lease.slot, map.get(), src4, n, src_normals4, times, t_begin,
                                                    t_end, begin_pose, guess_end, &prm, &r, QTR_MEM_HOST, info));
  return r;
}

// the pose at time t between (t_begin, begin_pose) and (t_end, end_pose) by the registration's rule
inline std::array<double, 16> ct_pose_at(double t_begin, double t_end, const double* begin_pose, const double* end_pose, double t) {
  std::array<double, 16> T{};
  if (qtr_voxel_map_ct_pose_at(t_begin, t_end, begin_pose, end_pose, t, T.data()) != QTR_OK)
    throw std::invalid_argument("[quatro_hip] qtr_voxel_map_ct_pose_at");
  return T;
}

}  // namespace quatro_hip
#endif  // QUATRO_VOXELMAP_CT_H
