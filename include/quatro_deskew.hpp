// quatro_deskew.hpp — motion compensation of a raw sweep over the process-wide handle of quatro_hip_cxx.hpp: free functions
// over qtr_deskew / qtr_deskew_pose_at and the definition of Keyframe::create_deskewed (declared in quatro_keyframe.hpp).  A
// header of its own because the calls are the extension library's (include/quatro_deskew.h): a program that includes only
// quatro_keyframe.hpp still links with -lquatro_hip; one that includes this header adds -lquatro_ext.  Host code only.
#ifndef QUATRO_DESKEW_H
#define QUATRO_DESKEW_H

#include <array>

#include "quatro_deskew.h"
#include "quatro_keyframe.hpp"

namespace quatro_hip {

inline int knot_count(const std::vector<double>& knot_times, const std::vector<double>& knot_poses) {
  if (knot_poses.size() != 16 * knot_times.size()) throw std::invalid_argument("[quatro_hip] deskew: 16 doubles per knot");
  return static_cast<int>(knot_times.size());
}

// The sweep xyz4 (n records of x, y, z, * in host memory) with the time of every point, carried into the sensor frame at
// t_ref under the knots (knot_times[k]: when; knot_poses[16 k ..]: row-major 4 x 4, sensor frame then -> a fixed frame).
// Returns the deskewed records; info (optional): points, skipped (non-finite, copied unchanged), extrapolated.
inline std::vector<float> deskew(const float* xyz4, const float* times, int n, const std::vector<double>& knot_times,
                                 const std::vector<double>& knot_poses, double t_ref, qtr_deskew_info* info = nullptr) {
  const int K = knot_count(knot_times, knot_poses);
  std::vector<float> out(static_cast<size_t>(n > 0 ? n : 0) * 4);
  SlotLease lease;
  check(default_handle(), qtr_deskew(default_handle(), lease.slot, xyz4, times, n, knot_times.data(), knot_poses.data(), K, t_ref,
                                     out.data(), QTR_MEM_HOST, info));
  return out;
}

// The pose the knots give at time t by the deskew's rule, row-major 4 x 4.  Host arithmetic only.
inline std::array<double, 16> pose_at(const std::vector<double>& knot_times, const std::vector<double>& knot_poses, double t) {
  std::array<double, 16> T{};
  if (qtr_deskew_pose_at(knot_times.data(), knot_poses.data(), knot_count(knot_times, knot_poses), t, T.data()) != QTR_OK)
    throw std::invalid_argument("[quatro_hip] pose_at: the knots are refused");
  return T;
}

inline Keyframe Keyframe::create_deskewed(const float* raw4, const float* times, int n, const std::vector<double>& knot_times,
                                          const std::vector<double>& knot_poses, double t_ref, const qtr_frontend_params& fp,
                                          qtr_deskew_info* info) {
  const int K = knot_count(knot_times, knot_poses);
  Keyframe out;
  SlotLease lease;
  check(default_handle(), qtr_keyframe_create_deskewed(default_handle(), lease.slot, raw4, times, n, knot_times.data(),
                                                       knot_poses.data(), K, t_ref, &fp, QTR_MEM_HOST, &out.kf_, info));
  return out;
}

}  // namespace quatro_hip
#endif  // QUATRO_DESKEW_H
