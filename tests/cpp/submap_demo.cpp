// submap_demo.cpp — a query registered against a submap, written against include/quatro_keyframe.hpp: the member scans
// become keyframes, Keyframe::merge fuses them under their poses into one keyframe, and the query is registered against it.
// usage: submap_demo poses.bin query.bin member0.bin member1.bin [...]
//   poses.bin: one row-major 4 x 4 of float64 per member (member frame -> submap frame); scans: float32 x,y,z,intensity
// Prints "submap members k n_points a n_voxels b", "valid v n_src a n_tgt b L c" and the 4x4 as the hex bits of every double.
#include <cstdio>
#include <cstring>
#include <vector>

#include "quatro_keyframe.hpp"

int main(int argc, char** argv) {
  if (argc < 5) {
    std::fprintf(stderr, "usage: %s poses.bin query.bin member0.bin member1.bin [...]\n", argv[0]);
    return 2;
  }
  const int K = argc - 3;
  std::vector<double> poses(16 * static_cast<size_t>(K));
  std::FILE* f = std::fopen(argv[1], "rb");
  if (!f || std::fread(poses.data(), 8, poses.size(), f) != poses.size()) {
    std::fprintf(stderr, "cannot read %d poses from %s\n", K, argv[1]);
    return 1;
  }
  std::fclose(f);
  qtr_frontend_params fp;
  qtr_default_frontend_params(&fp);
  qtr_params prm;
  qtr_demo_params(&prm);
  std::vector<quatro_hip::Keyframe> scans;  // [0]: the query, then the members
  std::vector<float> buffer(1000000);
  for (int a = 2; a < argc; ++a) {
    int n = 0;
    if (qtr_read_kitti_bin(argv[a], buffer.data(), 250000, &n) != QTR_OK) {
      std::fprintf(stderr, "cannot read %s\n", argv[a]);
      return 1;
    }
    scans.emplace_back(buffer.data(), n, fp);
  }
  std::vector<const quatro_hip::Keyframe*> members;
  for (int k = 0; k < K; ++k) members.push_back(&scans[1 + static_cast<size_t>(k)]);
  const quatro_hip::Keyframe submap = quatro_hip::Keyframe::merge(quatro_hip::default_handle(), -1, members, poses, fp);
  const qtr_keyframe_info info = submap.info();
  std::printf("submap members %d n_points %d n_voxels %d\n", K, info.n_points, info.n_voxels);
  const qtr_result r = quatro_hip::register_keyframes(scans[0], submap, fp, prm);
  std::printf("valid %d n_src %d n_tgt %d L %d\n", r.valid, r.n_src, r.n_tgt, r.n_corr);
  for (int i = 0; i < 4; ++i)
    for (int c = 0; c < 4; ++c) {
      unsigned long long b = 0;
      std::memcpy(&b, &r.T[4 * i + c], 8);
      std::printf("%016llx%c", b, c == 3 ? '\n' : ' ');
    }
  return 0;
}
