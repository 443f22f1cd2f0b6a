// deskew_demo.cpp — sweep deskew written against include/quatro_deskew.hpp: a raw sweep with the time of every point is
// deskewed under its knots, a keyframe is made of the same sweep in one call, and the pose at a time is asked for.
// usage: deskew_demo sweep.bin times.f32 knots.txt t_ref t_pose
//   (.bin = float32 x,y,z,* records; .f32 = one float32 per point; knots.txt = per knot 17 numbers: its time, then its
//   row-major 4x4 pose)
// Prints the deskew's counts and a checksum of the deskewed records (the exclusive-or of the bits of every float), the
// keyframe's counts with the checksum of its stored voxels, and the pose at t_pose.
#include <cstdio>
#include <cstring>
#include <fstream>
#include <string>
#include <vector>

#include "quatro_deskew.hpp"

static unsigned checksum(const std::vector<float>& v) {
  unsigned x = 0;
  for (float f : v) {
    unsigned b = 0;
    std::memcpy(&b, &f, 4);
    x ^= b;
  }
  return x;
}

int main(int argc, char** argv) {
  if (argc < 6) {
    std::fprintf(stderr, "usage: %s sweep.bin times.f32 knots.txt t_ref t_pose\n", argv[0]);
    return 2;
  }
  int n = 0;
  std::vector<float> sweep(1000000);
  if (qtr_read_kitti_bin(argv[1], sweep.data(), 250000, &n) != QTR_OK) throw std::runtime_error(std::string("cannot read ") + argv[1]);
  std::vector<float> times(static_cast<size_t>(n));
  {
    std::ifstream f(argv[2], std::ios::binary);
    f.read(reinterpret_cast<char*>(times.data()), static_cast<std::streamsize>(times.size() * 4));
    if (f.gcount() != static_cast<std::streamsize>(times.size() * 4)) throw std::runtime_error("times: one float per point");
  }
  std::vector<double> knot_times, knot_poses;
  {
    std::ifstream f(argv[3]);
    double t;
    while (f >> t) {
      knot_times.push_back(t);
      for (int k = 0; k < 16; ++k) {
        double v = 0;
        f >> v;
        knot_poses.push_back(v);
      }
    }
  }
  const double t_ref = std::stod(argv[4]);
  qtr_deskew_info info{};
  const std::vector<float> out = quatro_hip::deskew(sweep.data(), times.data(), n, knot_times, knot_poses, t_ref, &info);
  std::printf("deskew: points %d skipped %d extrapolated %d records %08x\n", info.n_points, info.n_skipped, info.n_extrapolated,
              checksum(out));
  qtr_frontend_params fp;
  qtr_default_frontend_params(&fp);
  qtr_deskew_info kinfo{};
  const quatro_hip::Keyframe kf =
      quatro_hip::Keyframe::create_deskewed(sweep.data(), times.data(), n, knot_times, knot_poses, t_ref, fp, &kinfo);
  const qtr_keyframe_info ki = kf.info();
  std::printf("keyframe: points %d voxels %d skipped %d voxels %08x\n", ki.n_points, ki.n_voxels, kinfo.n_skipped,
              checksum(kf.fetch(QTR_KF_VOX)));
  const std::array<double, 16> T = quatro_hip::pose_at(knot_times, knot_poses, std::stod(argv[5]));
  std::printf("pose:");
  for (double v : T) std::printf(" %.17g", v);
  std::printf("\n");
  return 0;
}
