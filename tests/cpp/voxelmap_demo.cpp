// voxelmap_demo.cpp — scan-to-map registration written against include/quatro_voxelmap.hpp: two voxelised scans with their
// normals are inserted into a Gaussian voxel map under their poses, a third is registered against the map.
// usage: voxelmap_demo voxel_size a.bin a_normals.bin pose_a.txt b.bin b_normals.bin pose_b.txt q.bin q_normals.bin guess.txt
//   (.bin = float32 x,y,z,* records; .txt = 16 numbers, row-major 4x4)
// Prints the map's voxel and member counts, then iterations, stop reason, correspondences, and the final 4x4, fitness and
// rmse as the hex bits of every double.
#include <cstdio>
#include <array>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "quatro_voxelmap.hpp"

static std::vector<float> getRecords(const char* path, int* n) {
  std::vector<float> buffer(1000000);
  if (qtr_read_kitti_bin(path, buffer.data(), 250000, n) != QTR_OK) throw std::runtime_error(std::string("cannot read ") + path);
  return buffer;
}

static std::array<double, 16> getPose(const char* path) {
  std::array<double, 16> p{};
  std::ifstream f(path);
  for (int k = 0; k < 16; ++k) f >> p[k];
  return p;
}

static void hex(double v, char end) {
  unsigned long long b = 0;
  std::memcpy(&b, &v, 8);
  std::printf("%016llx%c", b, end);
}

int main(int argc, char** argv) {
  if (argc < 11) {
    std::fprintf(stderr, "usage: %s voxel_size a.bin a_normals.bin pose_a.txt b.bin b_normals.bin pose_b.txt q.bin q_normals.bin guess.txt\n",
                 argv[0]);
    return 2;
  }
  quatro_hip::VoxelMap map(std::stod(argv[1]), 1 << 16);
  for (int k = 0; k < 2; ++k) {
    int n = 0, nn = 0;
    const std::vector<float> pts = getRecords(argv[2 + 3 * k], &n), nrm = getRecords(argv[3 + 3 * k], &nn);
    const std::array<double, 16> pose = getPose(argv[4 + 3 * k]);
    if (n != nn) throw std::runtime_error("points and normals differ in number");
    const qtr_voxel_map_insert_info i = map.insert(pts.data(), nrm.data(), n, pose.data());
    std::printf("insert %d: points %d members %d new %d touched %d\n", k, i.n_points, i.n_members, i.n_new_voxels, i.n_touched_voxels);
  }
  const qtr_voxel_map_info info = map.info();
  std::printf("map: voxels %d members %lld inserts %d cloud %zu\n", info.n_voxels, info.n_members, info.n_inserts,
              map.cloud().size() / 4);
  int n = 0, nn = 0;
  const std::vector<float> q = getRecords(argv[8], &n), qn = getRecords(argv[9], &nn);
  const std::array<double, 16> guess = getPose(argv[10]);
  const qtr_icp_result r = map.register_cloud(q.data(), qn.data(), n, guess.data());
  std::printf("iterations %d stop %d corr %d valid %d\n", r.iterations, r.stop_reason, r.n_corr, r.valid);
  for (int row = 0; row < 4; ++row)
    for (int c = 0; c < 4; ++c) hex(r.T[4 * row + c], c == 3 ? '\n' : ' ');
  hex(r.fitness, ' ');
  hex(r.rmse, '\n');
  return 0;
}
