// vgicp_demo.cpp — voxelised plane-to-plane (VGICP) refinement after a registration, written against
// include/quatro_icp.hpp: the target as one Gaussian per voxel of side setMaxCorrespondenceDistance, a lookup in place of
// the nearest-neighbour search.
// usage: vgicp_demo src.bin tgt.bin guess.txt [src_normals.bin tgt_normals.bin]
//   (.bin = float32 x,y,z,* records; guess.txt = 16 numbers, row-major 4x4; without the normal files both normal sets
//   are computed on the device at the default normal_radius)
// Prints iterations, stop reason, converged and the final 4x4 as the hex bits of every double.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "quatro_icp.hpp"

using PointT = pcl::PointXYZ;

static std::vector<float> getRecords(const char* path, int* n) {
  std::vector<float> buffer(1000000);
  if (qtr_read_kitti_bin(path, buffer.data(), 250000, n) != QTR_OK) throw std::runtime_error(std::string("cannot read ") + path);
  return buffer;
}

static pcl::PointCloud<PointT>::Ptr getCloud(const char* path) {
  pcl::PointCloud<PointT>::Ptr cloud(new pcl::PointCloud<PointT>());
  int n = 0;
  const std::vector<float> buffer = getRecords(path, &n);
  for (int i = 0; i < n; ++i) cloud->push_back(PointT(buffer[4 * i], buffer[4 * i + 1], buffer[4 * i + 2]));
  return cloud;
}

static std::vector<float> getNormals(const char* path) {
  int n = 0;
  const std::vector<float> buffer = getRecords(path, &n);
  std::vector<float> nxyz((size_t)3 * n);
  for (int i = 0; i < n; ++i)
    for (int a = 0; a < 3; ++a) nxyz[3 * i + a] = buffer[4 * i + a];
  return nxyz;
}

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s src.bin tgt.bin guess.txt [src_normals.bin tgt_normals.bin]\n", argv[0]);
    return 2;
  }
  auto src = getCloud(argv[1]);
  auto tgt = getCloud(argv[2]);
  Eigen::Matrix4d guess = Eigen::Matrix4d::Identity();
  std::ifstream gf(argv[3]);
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) gf >> guess(r, c);
  using Icp = quatro_hip::IterativeClosestPoint<PointT, PointT>;
  Icp icp(Icp::Method::VOXEL_PLANE_TO_PLANE);
  icp.setInputSource(src);
  icp.setInputTarget(tgt);
  if (argc > 5) {
    icp.setSourceNormals(getNormals(argv[4]));
    icp.setTargetNormals(getNormals(argv[5]));
  }
  icp.setMaxCorrespondenceDistance(1.0);  // (the voxel side)
  icp.setMaximumIterations(30);
  icp.setTransformationEpsilon(1e-7);
  icp.setEuclideanFitnessEpsilon(1e-6);
  pcl::PointCloud<PointT> aligned;
  icp.align(aligned, guess);
  const Eigen::Matrix4d T = icp.getFinalTransformation();
  std::printf("iterations %d stop %d converged %d fitness %.17g\n", icp.result().iterations, icp.result().stop_reason,
              icp.hasConverged() ? 1 : 0, icp.getFitnessScore());
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) {
      const double v = T(r, c);
      unsigned long long b = 0;
      std::memcpy(&b, &v, 8);
      std::printf("%016llx%c", b, c == 3 ? '\n' : ' ');
    }
  return 0;
}
