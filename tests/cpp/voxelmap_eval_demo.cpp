// voxelmap_eval_demo.cpp — scoring pose hypotheses written against include/quatro_voxelmap_eval.hpp: a voxelised scan with its
// normals is inserted into a Gaussian voxel map under its pose, and a query scan is evaluated against the map under a grid
// of hypotheses around a base pose (yaws -0.1, 0, 0.1 rad x offsets (0, 0), (1, 0), (0, 1) voxel sides) in one launch, then
// once more, alone, under the best of them.
// usage: voxelmap_eval_demo voxel_size a.bin a_normals.bin pose_a.txt q.bin q_normals.bin base.txt
//   (.bin = float32 x,y,z,* records; .txt = 16 numbers, row-major 4x4)
// Prints one line per hypothesis (n_source, correspondences, valid, and the hex bits of overlap and rmse), the winner, and the
// single call's information matrix as the hex bits of every double.
#include <array>
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "quatro_voxelmap_eval.hpp"

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
  if (argc < 8) {
    std::fprintf(stderr, "usage: %s voxel_size a.bin a_normals.bin pose_a.txt q.bin q_normals.bin base.txt\n", argv[0]);
    return 2;
  }
  const double side = std::stod(argv[1]);
  quatro_hip::VoxelMap map(side, 1 << 16);
  int n = 0, nn = 0;
  const std::vector<float> pts = getRecords(argv[2], &n), nrm = getRecords(argv[3], &nn);
  if (n != nn) throw std::runtime_error("points and normals differ in number");
  const std::array<double, 16> pose = getPose(argv[4]);
  map.insert(pts.data(), nrm.data(), n, pose.data());
  int nq = 0, nqn = 0;
  const std::vector<float> q = getRecords(argv[5], &nq), qn = getRecords(argv[6], &nqn);
  if (nq != nqn) throw std::runtime_error("points and normals differ in number");
  const std::array<double, 16> base = getPose(argv[7]);
  std::vector<qtr_vmap_reg_item> items;
  for (double yaw : {-0.1, 0.0, 0.1})
    for (const std::array<double, 2>& d : {std::array<double, 2>{0.0, 0.0}, std::array<double, 2>{side, 0.0}, std::array<double, 2>{0.0, side}}) {
      const std::array<double, 16> g = quatro_hip::hypothesis(base.data(), yaw, d[0], d[1]);
      items.push_back(quatro_hip::batch_item(q.data(), qn.data(), nq, g.data()));
    }
  const std::vector<qtr_vmap_eval_result> res = quatro_hip::evaluate_batch(map, items);
  for (size_t i = 0; i < res.size(); ++i) {
    std::printf("item %zu: source %d corr %d valid %d overlap ", i, res[i].n_source, res[i].n_corr, res[i].valid);
    hex(res[i].overlap, ' ');
    std::printf("rmse ");
    hex(res[i].rmse, '\n');
  }
  const int b = quatro_hip::best(res);
  std::printf("best %d\n", b);
  if (b >= 0) {
    const qtr_vmap_eval_result one = quatro_hip::evaluate(map, q.data(), qn.data(), nq, items[b].guess);
    for (int row = 0; row < 6; ++row)
      for (int c = 0; c < 6; ++c) hex(one.information[6 * row + c], c == 5 ? '\n' : ' ');
  }
  return 0;
}
