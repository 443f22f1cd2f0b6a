// quatro_voxelmap.hpp — the persistent Gaussian voxel map over the process-wide handle of quatro_hip_cxx.hpp: keyframes or
// clouds are inserted under poses (any number of them), scans are registered against the map with the voxelised
// plane-to-plane iteration, and the voxel means come back as the map cloud (qtr_voxel_map_*).  It is the global map after
// optimize_pose_graph (quatro_pgo.hpp), the target of scan-to-map odometry and of localisation in a finished map.  Poses
// are 16 row-major doubles (a quatro_hip::Pose of quatro_pgo.hpp passes as pose.data()).  Host code only; link with
// -lquatro_hip -lquatro_ext (the map's entry points are the extension library's, include/quatro_voxelmap.h).
#ifndef QUATRO_VOXELMAP_H
#define QUATRO_VOXELMAP_H

#include <stdexcept>
#include <vector>

#include "quatro_keyframe.hpp"
#include "quatro_voxelmap.h"

namespace quatro_hip {

inline qtr_icp_params default_map_icp_params() {
  qtr_icp_params p;
  qtr_default_icp_params(&p);
  p.method = QTR_ICP_VOXEL_PLANE_TO_PLANE;  // (the only method a map registration takes; the voxel side is the map's)
  return p;
}

// RAII owner of one qtr_voxel_map of default_handle(); move-only.  Registrations only read the map and may run from several
// threads at once; inserts and clear are the caller's to serialise.
class VoxelMap {
 public:
  VoxelMap() = default;
  explicit VoxelMap(double voxel_size, int capacity = 1 << 20) {
    qtr_voxel_map_params p;
    qtr_default_voxel_map_params(&p);
    p.voxel_size = voxel_size;
    p.capacity = capacity;
    check(default_handle(), qtr_voxel_map_create(default_handle(), &p, &m_));
  }
  ~VoxelMap() { reset(); }
  VoxelMap(VoxelMap&& o) noexcept : m_(o.m_) { o.m_ = nullptr; }
  VoxelMap& operator=(VoxelMap&& o) noexcept {
    if (this != &o) {
      reset();
      m_ = o.m_;
      o.m_ = nullptr;
    }
    return *this;
  }
  VoxelMap(const VoxelMap&) = delete;
  VoxelMap& operator=(const VoxelMap&) = delete;

  void reset() {
    if (m_) qtr_voxel_map_destroy(default_handle(), m_);
    m_ = nullptr;
  }
  explicit operator bool() const { return m_ != nullptr; }
  const qtr_voxel_map* get() const { return m_; }
  qtr_voxel_map_info info() const {
    qtr_voxel_map_info i{};
    check(default_handle(), qtr_voxel_map_get_info(m_, &i));
    return i;
  }
  void clear() {
    SlotLease lease;
    check(default_handle(), qtr_voxel_map_clear(default_handle(), lease.slot, m_));
  }
  // xyz4 / normals4: n records of 16 bytes each in host memory; pose: 16 doubles or nullptr (identity)
  qtr_voxel_map_insert_info insert(const float* xyz4, const float* normals4, int n, const double* pose = nullptr) {
    SlotLease lease;
    qtr_voxel_map_insert_info i{};
    check(default_handle(), qtr_voxel_map_insert(default_handle(), lease.slot, m_, xyz4, normals4, n, pose, QTR_MEM_HOST, &i));
    return i;
  }
  qtr_voxel_map_insert_info insert(const Keyframe& kf, const double* pose = nullptr) {
    SlotLease lease;
    qtr_voxel_map_insert_info i{};
    check(default_handle(), qtr_voxel_map_insert_keyframe(default_handle(), lease.slot, m_, kf.get(), pose, &i));
    return i;
  }
  qtr_icp_result register_cloud(const float* src4, const float* src_normals4, int n, const double* guess = nullptr,
                                const qtr_icp_params& prm = default_map_icp_params()) const {
    SlotLease lease;
    qtr_icp_result r{};
    check(default_handle(),
          qtr_voxel_map_register(default_handle(), lease.slot, m_, src4, n, src_normals4, guess, &prm, &r, QTR_MEM_HOST));
    return r;
  }
  qtr_icp_result register_keyframe(const Keyframe& kf, const double* guess = nullptr,
                                   const qtr_icp_params& prm = default_map_icp_params()) const {
    SlotLease lease;
    qtr_icp_result r{};
    check(default_handle(), qtr_voxel_map_register_keyframe(default_handle(), lease.slot, m_, kf.get(), guess, &prm, &r));
    return r;
  }
  // a fetch section (QTR_VMAP_*) as its element type: int for COORDS / COUNT, double for SUMS / RECORDS, float for CLOUD
  template <typename T>
  std::vector<T> fetch(int what) const {
    const long long bytes = qtr_voxel_map_fetch(default_handle(), m_, what, nullptr, 0);
    if (bytes < 0) throw std::invalid_argument("[quatro_hip] qtr_voxel_map_fetch");
    std::vector<T> out(static_cast<size_t>(bytes) / sizeof(T));
    if (bytes > 0 && qtr_voxel_map_fetch(default_handle(), m_, what, out.data(), static_cast<size_t>(bytes)) < 0)
      throw std::runtime_error("[quatro_hip] qtr_voxel_map_fetch");
    return out;
  }
  // the map as a point cloud: x, y, z = the voxel means, w = the member count
  std::vector<float> cloud() const { return fetch<float>(QTR_VMAP_CLOUD); }

 private:
  qtr_voxel_map* m_ = nullptr;
};

// The global map: every keyframe under its pose (16 doubles each, keyframe frame -> map frame), in order.
inline VoxelMap build_map(const std::vector<const Keyframe*>& keyframes, const std::vector<double>& poses, double voxel_size = 1.0,
                          int capacity = 1 << 20) {
  if (poses.size() != 16 * keyframes.size()) throw std::invalid_argument("[quatro_hip] build_map: 16 doubles per keyframe");
  VoxelMap m(voxel_size, capacity);
  for (size_t k = 0; k < keyframes.size(); ++k) m.insert(*keyframes[k], poses.data() + 16 * k);
  return m;
}

}  // namespace quatro_hip
#endif  // QUATRO_VOXELMAP_H
