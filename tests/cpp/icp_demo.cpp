// icp_demo.cpp — the refinement step after a registration, written against include/quatro_icp.hpp.
// usage: icp_demo src.bin tgt.bin guess.txt [point_to_point]
//   (.bin = float32 x,y,z,intensity records; guess.txt = 16 numbers, row-major 4x4)
// Prints iterations, stop reason, converged and the final 4x4 as the hex bits of every double.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "quatro_icp.hpp"

using PointT = pcl::PointXYZ;

static pcl::PointCloud<PointT>::Ptr getCloud(const char* path) {
  pcl::PointCloud<PointT>::Ptr cloud(new pcl::PointCloud<PointT>());
  std::vector<float> buffer(1000000);
  int n = 0;
  if (qtr_read_kitti_bin(path, buffer.data(), 250000, &n) != QTR_OK) throw std::runtime_error(std::string("cannot read ") + path);
  for (int i = 0; i < n; ++i) cloud->push_back(PointT(buffer[4 * i], buffer[4 * i + 1], buffer[4 * i + 2]));
  return cloud;
}

int main(int argc, char** argv) {
  if (argc < 4) {
    std::fprintf(stderr, "usage: %s src.bin tgt.bin guess.txt [point_to_point]\n", argv[0]);
    return 2;
  }
  auto src = getCloud(argv[1]);
  auto tgt = getCloud(argv[2]);
  Eigen::Matrix4d guess = Eigen::Matrix4d::Identity();
  std::ifstream gf(argv[3]);
  for (int r = 0; r < 4; ++r)
    for (int c = 0; c < 4; ++c) gf >> guess(r, c);
  using Icp = quatro_hip::IterativeClosestPoint<PointT, PointT>;
  const bool p2p = argc > 4 && std::string(argv[4]) == "point_to_point";
  Icp icp(p2p ? Icp::Method::POINT_TO_POINT : Icp::Method::POINT_TO_PLANE);
  icp.setInputSource(src);
  icp.setInputTarget(tgt);
  icp.setMaxCorrespondenceDistance(1.0);
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
