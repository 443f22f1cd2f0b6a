// eval_demo.cpp — a registration and its evaluation, written against include/quatro_eval.hpp: two scans become keyframes,
// are registered, and the result is evaluated keyframe against keyframe — what a caller does before the transform becomes
// an edge of a pose graph.
// usage: eval_demo source.bin target.bin max_correspondence_distance        (scans: float32 x,y,z,intensity)
// Prints "valid v n_source a n_corr b n_plane c", then overlap, sum_d2, inlier_rmse, plane_rmse and the two 6x6 matrices as
// the hex bits of every double.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "quatro_eval.hpp"

static void hex(const double* v, int n, int per_line) {
  for (int i = 0; i < n; ++i) {
    unsigned long long b = 0;
    std::memcpy(&b, &v[i], 8);
    std::printf("%016llx%c", b, (i + 1) % per_line == 0 ? '\n' : ' ');
  }
}

int main(int argc, char** argv) {
  if (argc != 4) {
    std::fprintf(stderr, "usage: %s source.bin target.bin max_correspondence_distance\n", argv[0]);
    return 2;
  }
  qtr_frontend_params fp;
  qtr_default_frontend_params(&fp);
  qtr_params prm;
  qtr_demo_params(&prm);
  std::vector<quatro_hip::Keyframe> scans;
  std::vector<float> buffer(1000000);
  for (int a = 1; a < 3; ++a) {
    int n = 0;
    if (qtr_read_kitti_bin(argv[a], buffer.data(), 250000, &n) != QTR_OK) {
      std::fprintf(stderr, "cannot read %s\n", argv[a]);
      return 1;
    }
    scans.emplace_back(buffer.data(), n, fp);
  }
  const qtr_result r = quatro_hip::register_keyframes(scans[0], scans[1], fp, prm);
  const qtr_eval_result e =
      quatro_hip::evaluate_registration(scans[0], scans[1], r.T, quatro_hip::default_eval_params(std::atof(argv[3])));
  std::printf("valid %d n_source %d n_corr %d n_plane %d\n", e.valid, e.n_source, e.n_corr, e.n_plane);
  const double s[4] = {e.overlap, e.sum_d2, e.inlier_rmse, e.plane_rmse};
  hex(s, 4, 4);
  hex(e.information, 36, 6);
  hex(e.hessian_plane, 36, 6);
  return 0;
}
