// voxelmap_ct_demo.cpp — continuous-time registration written against include/quatro_voxelmap_ct.hpp: a cloud with its normals
// is inserted into a Gaussian voxel map under a pose, then a raw sweep with the time of every point is registered against the
// map: its end pose is fitted, its begin pose held fixed.
// usage: voxelmap_ct_demo voxel_size a.bin a_normals.bin pose_a.txt q.bin q_normals.bin q_times.bin t_begin t_end begin.txt guess.txt
//   (.bin = float32 x,y,z,* records — q_times.bin carries the time of point i in the x of record i; .txt = 16 numbers,
//   row-major 4x4)
// Prints the insert's counts, the registration's counts, then iterations, stop reason, correspondences, the final 4x4 (the END
// pose), fitness and rmse, and the pose half-way through the sweep, as the hex bits of every double.
#include <array>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "quatro_voxelmap_ct.hpp"

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
  if (argc < 12) {
    std::fprintf(stderr,
                 "usage: %s voxel_size a.bin a_normals.bin pose_a.txt q.bin q_normals.bin q_times.bin t_begin t_end begin.txt guess.txt\n",
                 argv[0]);
    return 2;
  }
  quatro_hip::VoxelMap map(std::stod(argv[1]), 1 << 16);
  {
    int n = 0, nn = 0;
    const std::vector<float> pts = getRecords(argv[2], &n), nrm = getRecords(argv[3], &nn);
    const std::array<double, 16> pose = getPose(argv[4]);
    if (n != nn) throw std::runtime_error("points and normals differ in number");
    const qtr_voxel_map_insert_info i = map.insert(pts.data(), nrm.data(), n, pose.data());
    std::printf("insert: points %d members %d new %d touched %d\n", i.n_points, i.n_members, i.n_new_voxels, i.n_touched_voxels);
  }
  int n = 0, nn = 0, nt = 0;
  const std::vector<float> q = getRecords(argv[5], &n), qn = getRecords(argv[6], &nn), qt = getRecords(argv[7], &nt);
  if (n != nn || n != nt) throw std::runtime_error("points, normals and times differ in number");
  std::vector<float> times(static_cast<size_t>(n));
  for (int i = 0; i < n; ++i) times[i] = qt[4 * static_cast<size_t>(i)];
  const double t_begin = std::stod(argv[8]), t_end = std::stod(argv[9]);
  const std::array<double, 16> begin = getPose(argv[10]), guess = getPose(argv[11]);
  qtr_vmap_ct_info info{};
  const qtr_icp_result r = quatro_hip::register_ct(map, q.data(), qn.data(), times.data(), n, t_begin, t_end, begin.data(),
                                                   guess.data(), quatro_hip::default_map_icp_params(), &info);
  std::printf("sweep: points %d skipped %d extrapolated %d\n", info.n_points, info.n_skipped, info.n_extrapolated);
  std::printf("iterations %d stop %d corr %d valid %d\n", r.iterations, r.stop_reason, r.n_corr, r.valid);
  for (int row = 0; row < 4; ++row)
    for (int c = 0; c < 4; ++c) hex(r.T[4 * row + c], c == 3 ? '\n' : ' ');
  hex(r.fitness, ' ');
  hex(r.rmse, '\n');
  const std::array<double, 16> mid = quatro_hip::ct_pose_at(t_begin, t_end, begin.data(), r.T, 0.5 * (t_begin + t_end));
  for (int row = 0; row < 4; ++row)
    for (int c = 0; c < 4; ++c) hex(mid[4 * row + c], c == 3 ? '\n' : ' ');
  return 0;
}
