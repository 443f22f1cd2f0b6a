// keyframe_demo.cpp — an odometry chain written against include/quatro_keyframe.hpp: every scan's front end runs once,
// pair (k, k + 1) is registered keyframe against keyframe with tuple-test seed k.
// usage: keyframe_demo scan0.bin scan1.bin [scan2.bin ...]   (.bin = float32 x,y,z,intensity records)
// Prints, per pair, a line "pair k valid v n_src a n_tgt b L c" and the 4x4 as the hex bits of every double.
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "quatro_keyframe.hpp"

int main(int argc, char** argv) {
  if (argc < 3) {
    std::fprintf(stderr, "usage: %s scan0.bin scan1.bin [...]\n", argv[0]);
    return 2;
  }
  qtr_frontend_params fp;
  qtr_default_frontend_params(&fp);
  qtr_params prm;
  qtr_demo_params(&prm);
  std::vector<quatro_hip::Keyframe> chain;
  std::vector<float> buffer(1000000);
  for (int a = 1; a < argc; ++a) {
    int n = 0;
    if (qtr_read_kitti_bin(argv[a], buffer.data(), 250000, &n) != QTR_OK) {
      std::fprintf(stderr, "cannot read %s\n", argv[a]);
      return 1;
    }
    chain.emplace_back(buffer.data(), n, fp);
  }
  for (size_t k = 0; k + 1 < chain.size(); ++k) {
    fp.seed = k;
    const qtr_result r = quatro_hip::register_keyframes(chain[k], chain[k + 1], fp, prm);
    std::printf("pair %zu valid %d n_src %d n_tgt %d L %d\n", k, r.valid, r.n_src, r.n_tgt, r.n_corr);
    for (int i = 0; i < 4; ++i)
      for (int c = 0; c < 4; ++c) {
        unsigned long long b = 0;
        std::memcpy(&b, &r.T[4 * i + c], 8);
        std::printf("%016llx%c", b, c == 3 ? '\n' : ' ');
      }
  }
  return 0;
}
