// voxelmap_keep_demo.cpp — the voxel map's upkeep written against include/quatro_voxelmap_keep.hpp: a voxelised scan with its
// normals is inserted under a pose, the map is evicted around a centre, and what is left is restored into a second, smaller
// map.
// usage: voxelmap_keep_demo voxel_size a.bin a_normals.bin pose_a.txt cx cy cz radius capacity
//   (.bin = float32 x,y,z,* records; .txt = 16 numbers, row-major 4x4)
// Prints the map's counts before and after the eviction, what left, the copy's counts, and a checksum of the copy's sums
// (the exclusive-or of the bits of every double).
#include <array>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "quatro_voxelmap_keep.hpp"

static std::vector<float> getRecords(const char* path, int* n) {
  std::vector<float> buffer(1000000);
  if (qtr_read_kitti_bin(path, buffer.data(), 250000, n) != QTR_OK) throw std::runtime_error(std::string("cannot read ") + path);
  return buffer;
}

static void print(const char* what, const qtr_voxel_map_info& i) {
  std::printf("%s: voxels %d members %lld inserts %d\n", what, i.n_voxels, i.n_members, i.n_inserts);
}

int main(int argc, char** argv) {
  if (argc < 10) {
    std::fprintf(stderr, "usage: %s voxel_size a.bin a_normals.bin pose_a.txt cx cy cz radius capacity\n", argv[0]);
    return 2;
  }
  quatro_hip::VoxelMap map(std::stod(argv[1]), 1 << 16);
  int n = 0, nn = 0;
  const std::vector<float> pts = getRecords(argv[2], &n), nrm = getRecords(argv[3], &nn);
  if (n != nn) throw std::runtime_error("points and normals differ in number");
  std::array<double, 16> pose{};
  {
    std::ifstream f(argv[4]);
    for (int k = 0; k < 16; ++k) f >> pose[k];
  }
  map.insert(pts.data(), nrm.data(), n, pose.data());
  print("map", map.info());
  const double centre[3] = {std::stod(argv[5]), std::stod(argv[6]), std::stod(argv[7])};
  const qtr_voxel_map_evict_info e = quatro_hip::evict(map, centre, std::stod(argv[8]));
  std::printf("evict: kept %d evicted %d members %lld\n", e.n_kept, e.n_evicted, e.n_members_evicted);
  print("window", map.info());
  const quatro_hip::VoxelMap copy = quatro_hip::copy_map(map, std::stoi(argv[9]));
  print("copy", copy.info());
  unsigned long long x = 0;
  for (double v : copy.fetch<double>(QTR_VMAP_SUMS)) {
    unsigned long long b = 0;
    std::memcpy(&b, &v, 8);
    x ^= b;
  }
  std::printf("sums %016llx cloud %zu\n", x, copy.cloud().size() / 4);
  return 0;
}
