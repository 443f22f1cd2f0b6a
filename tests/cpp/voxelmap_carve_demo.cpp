// voxelmap_carve_demo.cpp — visibility carving written against include/quatro_voxelmap_carve.hpp: a voxelised scan with its
// normals is inserted under a pose, and the map is carved with a later scan taken at another pose.
// usage: voxelmap_carve_demo voxel_size a.bin a_normals.bin pose_a.txt scan.bin pose_scan.txt rows cols fov_up fov_down window
//   (.bin = float32 x,y,z,* records; .txt = 16 numbers, row-major 4x4)
// Prints the map's counts before the carve, what the carve reports, the counts after it, and a checksum of the sums that are
// left (the exclusive-or of the bits of every double).
#include <array>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "quatro_voxelmap_carve.hpp"

static std::vector<float> getRecords(const char* path, int* n) {
  std::vector<float> buffer(1000000);
  if (qtr_read_kitti_bin(path, buffer.data(), 250000, n) != QTR_OK) throw std::runtime_error(std::string("cannot read ") + path);
  return buffer;
}

static std::array<double, 16> getPose(const char* path) {
  std::array<double, 16> pose{};
  std::ifstream f(path);
  for (int k = 0; k < 16; ++k) f >> pose[k];
  return pose;
}

static void print(const char* what, const qtr_voxel_map_info& i) {
  std::printf("%s: voxels %d members %lld inserts %d\n", what, i.n_voxels, i.n_members, i.n_inserts);
}

int main(int argc, char** argv) {
  if (argc < 12) {
    std::fprintf(stderr, "usage: %s voxel_size a.bin a_normals.bin pose_a.txt scan.bin pose_scan.txt rows cols fov_up fov_down window\n",
                 argv[0]);
    return 2;
  }
  quatro_hip::VoxelMap map(std::stod(argv[1]), 1 << 16);
  int n = 0, nn = 0, ns = 0;
  const std::vector<float> pts = getRecords(argv[2], &n), nrm = getRecords(argv[3], &nn);
  if (n != nn) throw std::runtime_error("points and normals differ in number");
  const std::array<double, 16> pose = getPose(argv[4]);
  map.insert(pts.data(), nrm.data(), n, pose.data());
  print("map", map.info());
  const std::vector<float> scan = getRecords(argv[5], &ns);
  const std::array<double, 16> at = getPose(argv[6]);
  qtr_carve_params prm = quatro_hip::default_carve_params();
  prm.rows = std::stoi(argv[7]);
  prm.cols = std::stoi(argv[8]);
  prm.fov_up_deg = std::stod(argv[9]);
  prm.fov_down_deg = std::stod(argv[10]);
  prm.window = std::stoi(argv[11]);
  prm.min_range = 0.5;
  const qtr_voxel_map_carve_info c = quatro_hip::carve(map, scan.data(), ns, at.data(), prm);
  std::printf("carve: kept %d carved %d tested %d members %lld\n", c.n_kept, c.n_carved, c.n_tested, c.n_members_carved);
  print("carved", map.info());
  unsigned long long x = 0;
  for (double v : map.fetch<double>(QTR_VMAP_SUMS)) {
    unsigned long long b = 0;
    std::memcpy(&b, &v, 8);
    x ^= b;
  }
  std::printf("sums %016llx cloud %zu\n", x, map.cloud().size() / 4);
  return 0;
}
