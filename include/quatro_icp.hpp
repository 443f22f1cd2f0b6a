// quatro_icp.hpp — pcl::IterativeClosestPoint's surface (setInputSource / setInputTarget / the convergence knobs /
// align / hasConverged / getFitnessScore / getFinalTransformation) over qtr_icp: the 6-DoF refinement that normally
// follows a Quatro registration (Quatro recovers yaw and translation; roll and pitch come only from estimated_RyRx_).
// Point-to-plane by default (pcl::IterativeClosestPointWithNormals; target normals at normal_radius unless
// setTargetNormals gives them), point-to-point or plane-to-plane (Generalized ICP: qtr_gicp with the normals of both
// clouds, given by setSourceNormals / setTargetNormals or computed at normal_radius) or its voxelised form (VGICP: the voxel
// side is setMaxCorrespondenceDistance, normals as for plane-to-plane) on request.  Host code only; link
// with -lquatro_hip.  Compiles with the
// built-in stand-ins of quatro.hpp and against PCL / Eigen (QUATRO_HAVE_PCL).
#ifndef QUATRO_ICP_H
#define QUATRO_ICP_H

#include <vector>

#include "quatro.hpp"

namespace quatro_hip {

template <typename PointSource, typename PointTarget>
class IterativeClosestPoint {
 public:
  using PointCloudSource = pcl::PointCloud<PointSource>;
  using PointCloudTarget = pcl::PointCloud<PointTarget>;
  using PointCloudSourceConstPtr = typename PointCloudSource::ConstPtr;
  using PointCloudTargetConstPtr = typename PointCloudTarget::ConstPtr;
  enum class Method {
    POINT_TO_PLANE = QTR_ICP_POINT_TO_PLANE,
    POINT_TO_POINT = QTR_ICP_POINT_TO_POINT,
    PLANE_TO_PLANE = QTR_ICP_PLANE_TO_PLANE,
    VOXEL_PLANE_TO_PLANE = QTR_ICP_VOXEL_PLANE_TO_PLANE  // (VGICP: routed like PLANE_TO_PLANE)
  };

  explicit IterativeClosestPoint(Method method = Method::POINT_TO_PLANE) {
    qtr_default_icp_params(&prm_);
    prm_.method = static_cast<int>(method);
    final_ = Eigen::Matrix4d::Identity();
  }

  void setInputSource(const PointCloudSourceConstPtr& cloud) {
    input_ = cloud;
    src_normals_.clear();
  }
  // nx, ny, nz per source point, source frame (plane-to-plane); not called: computed at normal_radius on the device
  void setSourceNormals(const std::vector<float>& nxyz) {
    src_normals_.assign(nxyz.size() / 3 * 4, 0.f);
    for (size_t i = 0; i < nxyz.size() / 3; ++i)
      for (int a = 0; a < 3; ++a) src_normals_[4 * i + a] = nxyz[3 * i + a];
  }
  void setInputTarget(const PointCloudTargetConstPtr& cloud) {
    target_ = cloud;
    normals_.clear();
  }
  // nx, ny, nz per target point (point-to-plane, plane-to-plane); not called: computed at normal_radius on the device
  void setTargetNormals(const std::vector<float>& nxyz) {
    normals_.assign(nxyz.size() / 3 * 4, 0.f);
    for (size_t i = 0; i < nxyz.size() / 3; ++i)
      for (int a = 0; a < 3; ++a) normals_[4 * i + a] = nxyz[3 * i + a];
  }
  void setMaxCorrespondenceDistance(double d) { prm_.max_correspondence_distance = d; }
  void setMaximumIterations(int n) { prm_.max_iterations = n; }
  void setTransformationEpsilon(double e) { prm_.transformation_epsilon = e; }
  void setEuclideanFitnessEpsilon(double e) { prm_.euclidean_fitness_epsilon = e; }
  void setNormalRadius(float r) { prm_.normal_radius = r; }
  double getMaxCorrespondenceDistance() const { return prm_.max_correspondence_distance; }
  int getMaximumIterations() const { return prm_.max_iterations; }

  // pcl::Registration::align(output, guess): output = the source under the final transformation
  void align(PointCloudSource& output, const Eigen::Matrix4d& guess = Eigen::Matrix4d::Identity()) {
    if (!input_ || !target_) throw std::invalid_argument("[IterativeClosestPoint] input clouds are not set");
    qtr_handle* h = default_handle();
    SlotLease slot_lease;
    double g[16];
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) g[4 * r + c] = guess(r, c);
    const int ns = static_cast<int>(input_->points.size()), nt = static_cast<int>(target_->points.size());
    const bool given = !normals_.empty() && normals_.size() == 4 * target_->points.size();
    int rc;
    if (prm_.method == QTR_ICP_PLANE_TO_PLANE || prm_.method == QTR_ICP_VOXEL_PLANE_TO_PLANE) {
      const bool src_given = !src_normals_.empty() && src_normals_.size() == 4 * input_->points.size();
      rc = qtr_gicp(h, slot_lease.slot, xyz4(input_->points), ns, src_given ? src_normals_.data() : nullptr,
                    xyz4(target_->points), nt, given ? normals_.data() : nullptr, g, &prm_, &res_, QTR_MEM_HOST);
    } else {
      rc = qtr_icp(h, slot_lease.slot, xyz4(input_->points), ns, xyz4(target_->points), nt,
                   given ? normals_.data() : nullptr, g, &prm_, &res_, QTR_MEM_HOST);
    }
    check(h, rc);
    for (int r = 0; r < 4; ++r)
      for (int c = 0; c < 4; ++c) final_(r, c) = res_.T[4 * r + c];
    output = *input_;
    for (auto& p : output.points) {
      const double x = p.x, y = p.y, z = p.z;
      p.x = static_cast<float>(res_.T[0] * x + res_.T[1] * y + res_.T[2] * z + res_.T[3]);
      p.y = static_cast<float>(res_.T[4] * x + res_.T[5] * y + res_.T[6] * z + res_.T[7]);
      p.z = static_cast<float>(res_.T[8] * x + res_.T[9] * y + res_.T[10] * z + res_.T[11]);
    }
  }

  bool hasConverged() const { return res_.converged != 0; }
  // mean squared distance of the last iteration's correspondences (DBL_MAX without any, like pcl)
  double getFitnessScore() const { return res_.fitness; }
  Eigen::Matrix4d getFinalTransformation() const { return final_; }
  const qtr_icp_result& result() const { return res_; }

 private:
  PointCloudSourceConstPtr input_;
  PointCloudTargetConstPtr target_;
  std::vector<float> normals_, src_normals_;
  qtr_icp_params prm_;
  qtr_icp_result res_{};
  Eigen::Matrix4d final_;
};

}  // namespace quatro_hip

#endif  // QUATRO_ICP_H
