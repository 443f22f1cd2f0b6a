// pgo_demo.cpp — a pose graph optimised through include/quatro_pgo.hpp.
// usage: pgo_demo graph.bin
// graph.bin: int32 N, int32 E, float64 line_process_weight, then poses (16 N float64), fixed (N bytes), src (E int32), dst
// (E int32), Z (16 E float64), information (36 E float64), uncertain (E bytes).
// Prints "status s valid v iterations i accepted a pcg p stop r pruned n", then objective_initial, objective_final,
// lambda_final, the poses and the weights as the hex bits of every double.
#include <cstdio>
#include <cstring>
#include <vector>

#include "quatro_pgo.hpp"

static void hex(const double* v, int n, int per_line) {
  for (int i = 0; i < n; ++i) {
    unsigned long long b = 0;
    std::memcpy(&b, &v[i], 8);
    std::printf("%016llx%c", b, ((i + 1) % per_line == 0 || i + 1 == n) ? '\n' : ' ');
  }
}

int main(int argc, char** argv) {
  if (argc != 2) {
    std::fprintf(stderr, "usage: %s graph.bin\n", argv[0]);
    return 2;
  }
  std::FILE* f = std::fopen(argv[1], "rb");
  int N = 0, E = 0;
  double mu = 0.0;
  if (!f || std::fread(&N, 4, 1, f) != 1 || std::fread(&E, 4, 1, f) != 1 || std::fread(&mu, 8, 1, f) != 1 || N < 1 || E < 0 ||
      N > QTR_PGO_MAX_NODES || E > QTR_PGO_MAX_EDGES) {
    std::fprintf(stderr, "cannot read %s\n", argv[1]);
    return 1;
  }
  std::vector<quatro_hip::Pose> poses(N), Z(E);
  std::vector<quatro_hip::Information> info(E);
  std::vector<unsigned char> fixed(N), unc(E);
  std::vector<int> src(E), dst(E);
  bool ok = std::fread(poses.data(), 128, N, f) == (size_t)N && std::fread(fixed.data(), 1, N, f) == (size_t)N;
  ok = ok && std::fread(src.data(), 4, E, f) == (size_t)E && std::fread(dst.data(), 4, E, f) == (size_t)E;
  ok = ok && std::fread(Z.data(), 128, E, f) == (size_t)E && std::fread(info.data(), 288, E, f) == (size_t)E;
  ok = ok && std::fread(unc.data(), 1, E, f) == (size_t)E;
  std::fclose(f);
  if (!ok) {
    std::fprintf(stderr, "%s is short\n", argv[1]);
    return 1;
  }
  quatro_hip::PoseGraph g;
  for (int i = 0; i < N; ++i) g.add_node(poses[i], fixed[i] != 0);
  for (int e = 0; e < E; ++e) g.add_edge(src[e], dst[e], Z[e].data(), info[e].data(), unc[e] != 0);
  const quatro_hip::PgoOutcome o = g.optimize(quatro_hip::default_pgo_params(mu));
  const qtr_pgo_result& r = o.result;
  std::printf("status %d valid %d iterations %d accepted %d pcg %d stop %d pruned %d\n", r.status, r.valid, r.iterations,
              r.accepted, r.pcg_iterations_total, r.stop_reason, (int)o.pruned.size());
  const double s[3] = {r.objective_initial, r.objective_final, r.lambda_final};
  hex(s, 3, 3);
  hex(g.poses()[0].data(), 16 * N, 16);
  hex(o.weights.data(), E, 8);
  return 0;
}
