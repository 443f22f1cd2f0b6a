// quatro_eval.hpp — evaluation of a registration over the process-wide handle of quatro_hip_cxx.hpp: how much of the source
// lies on the target under T (overlap, inlier RMSE: Open3D's evaluate_registration), the 6x6 information matrix of the
// pose-graph edge (get_information_matrix_from_point_clouds) and the point-to-plane Hessian at T.  The clouds stay where
// they are: host records are staged once, keyframes are read in place.  Host code only; link with -lquatro_hip.
#ifndef QUATRO_EVAL_H
#define QUATRO_EVAL_H

#include "quatro_keyframe.hpp"

namespace quatro_hip {

inline qtr_eval_params default_eval_params(double max_correspondence_distance = 1.0) {
  qtr_eval_params p;
  qtr_default_eval_params(&p);
  p.max_correspondence_distance = max_correspondence_distance;
  return p;
}

// src4 / tgt4: n records of 16 bytes (x, y, z, *) in host memory; tgt_normals4: n_t records or nullptr (no plane sums);
// T: row-major 4 x 4, maps source into target.
inline qtr_eval_result evaluate_registration(const float* src4, int n_s, const float* tgt4, int n_t, const float* tgt_normals4,
                                             const double T[16], const qtr_eval_params& prm = default_eval_params()) {
  SlotLease lease;
  qtr_eval_result res{};
  check(default_handle(), qtr_evaluate(default_handle(), lease.slot, src4, n_s, tgt4, n_t, tgt_normals4, T, &prm, &res,
                                       QTR_MEM_HOST));
  return res;
}

// Two keyframes: the voxels of both and the target's normals, read where they lie.
inline qtr_eval_result evaluate_registration(const Keyframe& source, const Keyframe& target, const double T[16],
                                             const qtr_eval_params& prm = default_eval_params()) {
  SlotLease lease;
  qtr_eval_result res{};
  check(default_handle(), qtr_evaluate_keyframes(default_handle(), lease.slot, source.get(), target.get(), T, &prm, &res));
  return res;
}

}  // namespace quatro_hip
#endif  // QUATRO_EVAL_H
