// quatro_keyframe.hpp — keyframes over the process-wide handle of quatro_hip_cxx.hpp: a scan's front end (voxel grid,
// normals, FPFH) is run once and kept on the device; registrations then run keyframe against keyframe.  Loop closing
// registers one query against many candidates (register_one_to_many), odometry reuses scan k's keyframe as the source of
// pair (k, k + 1) — the reference's FPFHManager::is_odometry_test_ (include/fpfh_manager.hpp:111-118) without carrying
// descriptors through host vectors.  Results are bit-identical to the raw-scan path (qtr_register_pair).
// Keyframe::merge fuses keyframes under their poses into one submap keyframe, which every call here takes like any other.
// Host code only; link with -lquatro_hip.
#ifndef QUATRO_KEYFRAME_H
#define QUATRO_KEYFRAME_H

#include <stdexcept>
#include <utility>
#include <vector>

#include "quatro_hip_cxx.hpp"

struct qtr_deskew_info;  // (include/quatro_deskew.h)

namespace quatro_hip {

// RAII owner of one qtr_keyframe of default_handle(); move-only, read-only once made.
class Keyframe {
 public:
  Keyframe() = default;
  // xyz4: n records of 16 bytes (x, y, z, *) in host memory — pcl::PointXYZ, the KITTI .bin record
  Keyframe(const float* xyz4, int n, const qtr_frontend_params& fp) {
    SlotLease lease;
    check(default_handle(), qtr_keyframe_create(default_handle(), lease.slot, xyz4, n, &fp, QTR_MEM_HOST, &kf_));
  }
  ~Keyframe() { reset(); }
  Keyframe(Keyframe&& o) noexcept : kf_(o.kf_) { o.kf_ = nullptr; }
  Keyframe& operator=(Keyframe&& o) noexcept {
    if (this != &o) {
      reset();
      kf_ = o.kf_;
      o.kf_ = nullptr;
    }
    return *this;
  }
  Keyframe(const Keyframe&) = delete;
  Keyframe& operator=(const Keyframe&) = delete;

  void reset() {
    if (kf_) qtr_keyframe_destroy(default_handle(), kf_);
    kf_ = nullptr;
  }
  explicit operator bool() const { return kf_ != nullptr; }
  const qtr_keyframe* get() const { return kf_; }
  qtr_keyframe_info info() const {
    qtr_keyframe_info i{};
    check(default_handle(), qtr_keyframe_get_info(kf_, &i));
    return i;
  }
  // A submap: the members' stored voxels, member k moved by poses[16 * k .. 16 * k + 15] (row-major 4 x 4, rows 0 - 2 used;
  // poses empty: identities), fused on the device into one keyframe with the submap's own fp (qtr_keyframe_merge).  slot < 0:
  // a leased slot.
  static Keyframe merge(qtr_handle* handle, int slot, const std::vector<const Keyframe*>& members,
                        const std::vector<double>& poses, const qtr_frontend_params& fp) {
    if (!poses.empty() && poses.size() != 16 * members.size())
      throw std::invalid_argument("[quatro_hip] Keyframe::merge: 16 doubles per member");
    if (handle != default_handle()) throw std::invalid_argument("[quatro_hip] Keyframe::merge: not the process-wide handle");
    std::vector<const qtr_keyframe*> kfs(members.size());
    for (size_t k = 0; k < members.size(); ++k) kfs[k] = members[k] ? members[k]->get() : nullptr;
    Keyframe out;
    const double* p = poses.empty() ? nullptr : poses.data();
    if (slot >= 0) {
      check(handle, qtr_keyframe_merge(handle, slot, kfs.data(), p, static_cast<int>(kfs.size()), &fp, &out.kf_));
    } else {
      SlotLease lease;
      check(handle, qtr_keyframe_merge(handle, lease.slot, kfs.data(), p, static_cast<int>(kfs.size()), &fp, &out.kf_));
    }
    return out;
  }
  // A keyframe of a RAW sweep of a moving sensor, deskewed on the device on its way (qtr_keyframe_create_deskewed): times = n
  // floats, the time of every point; K = knot_times.size() knots, knot_poses 16 doubles each; info (optional) receives the
  // deskew's counts.  DEFINED in quatro_deskew.hpp: a program that calls it includes that header and adds -lquatro_ext.
  static Keyframe create_deskewed(const float* raw4, const float* times, int n, const std::vector<double>& knot_times,
                                  const std::vector<double>& knot_poses, double t_ref, const qtr_frontend_params& fp,
                                  qtr_deskew_info* info = nullptr);
  // QTR_KF_VOX / _NORMALS / _FPFH / _MEAN as floats
  std::vector<float> fetch(int what) const {
    const long long bytes = qtr_keyframe_fetch(default_handle(), kf_, what, nullptr, 0);
    if (bytes < 0) throw std::invalid_argument("[quatro_hip] qtr_keyframe_fetch");
    std::vector<float> out(static_cast<size_t>(bytes) / 4);
    if (bytes > 0) qtr_keyframe_fetch(default_handle(), kf_, what, out.data(), static_cast<size_t>(bytes));
    return out;
  }

 private:
  qtr_keyframe* kf_ = nullptr;
};

// One registration, keyframe against keyframe, on a leased slot.  A "clique too small" outcome returns with valid = 0.
inline qtr_result register_keyframes(const Keyframe& src, const Keyframe& tgt, const qtr_frontend_params& fp,
                                     const qtr_params& prm) {
  SlotLease lease;
  qtr_result res{};
  check(default_handle(), qtr_register_keyframes(default_handle(), lease.slot, src.get(), tgt.get(), &fp, &prm, &res, nullptr,
                                                 nullptr, 0));
  return res;
}

// One query against K candidates as one batched job (every slot of the process-wide handle: do not run other wrapper calls
// meanwhile).  Returns the records in candidate order; *best (optional) receives the index of the valid record with the
// most final inliers, ties to the lowest index, -1 when none is valid.
inline std::vector<qtr_result> register_one_to_many(const Keyframe& query, const std::vector<const Keyframe*>& candidates,
                                                    const qtr_frontend_params& fp, const qtr_params& prm, int* best = nullptr) {
  std::vector<qtr_kf_pair_desc> pairs(candidates.size());
  std::vector<qtr_result> out(candidates.size());
  for (size_t k = 0; k < candidates.size(); ++k) pairs[k] = qtr_kf_pair_desc{query.get(), candidates[k]->get(), fp.seed, nullptr, nullptr, 0};
  qtr_handle* h = default_handle();
  check(h, qtr_submit_batch_keyframes(h, pairs.data(), static_cast<int>(pairs.size()), &fp, &prm, nullptr, out.data(), nullptr));
  check(h, qtr_wait(h));
  if (best) {
    *best = -1;
    for (size_t k = 0; k < out.size(); ++k)
      if (out[k].valid && (*best < 0 || out[k].n_final > out[static_cast<size_t>(*best)].n_final)) *best = static_cast<int>(k);
  }
  return out;
}

}  // namespace quatro_hip
#endif  // QUATRO_KEYFRAME_H
