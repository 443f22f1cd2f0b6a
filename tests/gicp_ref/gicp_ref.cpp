// gicp_ref.cpp — host restatement of the device loop's plane-to-plane method (quatro_amd/csrc/icp.hip, d_icp_iter<true>)
// for the tests: the same include/qtr_icp_math.h arithmetic (qtr_icp_gicp_terms, qtr_icp_step), the same fixed-shape
// sums, and a hash grid of its own for the nearest-neighbour search (the search's result does not depend on the grid:
// nearest binary64 d^2 within reach, ties to the lowest target index).  Built by the tests with g++ -O2 -ffp-contract=off
// -shared -fPIC.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "qtr_icp_math.h"

namespace {
// cells of side >= max_d from the origin: a point within max_d of q lies in one of the 27 cells around q's
struct Cells {
  double side = 1;
  // (three whole indices per key, so a scene may lie any number of cells from the origin: map coordinates do)
  struct Key {
    int64_t x, y, z;
    bool operator==(const Key& o) const { return x == o.x && y == o.y && z == o.z; }
  };
  struct Hash {
    size_t operator()(const Key& k) const {
      uint64_t h = (uint64_t)k.x * 0x9E3779B97F4A7C15ull;
      h = (h ^ (h >> 29) ^ (uint64_t)k.y) * 0xBF58476D1CE4E5B9ull;
      h = (h ^ (h >> 32) ^ (uint64_t)k.z) * 0x94D049BB133111EBull;
      return (size_t)(h ^ (h >> 31));
    }
  };
  std::unordered_map<Key, std::vector<int>, Hash> at;
  static Key key(int64_t x, int64_t y, int64_t z) { return Key{x, y, z}; }
  double cell(double x) const { return std::floor(x / side); }
};
}  // namespace

extern "C" int gicp_ref_run(const float* src4, int ns, const float* src_nrm4, const float* tgt4, int nt, const float* tgt_nrm4,
                            const double* guess, double max_d, double teps, double feps, int max_iter, int min_corr,
                            double* T_out, int* info /* iterations, reason, valid, converged, n_corr */,
                            double* fit_rmse /* 2 */, double* trace /* max_iter x 18 */,
                            int* corr_at /* ns or null */, int corr_iter /* evaluation whose correspondences to keep */) {
  QtrIcpCfg cfg;
  cfg.max_d2 = max_d * max_d;
  cfg.trans_eps = teps;
  cfg.fit_eps = feps;
  cfg.max_iterations = max_iter;
  cfg.method = 2;
  cfg.min_corr = min_corr > 0 ? min_corr : 4;
  cfg.pad = 0;
  QtrIcpState st;
  qtr_icp_init(&st, guess);
  st.reason = QTR_ICP_STOP_TOO_FEW;
  Cells g;
  g.side = max_d * 1.001;
  for (int j = 0; j < nt; ++j) {  // the finite target points, ascending inside every cell
    const float* t = tgt4 + 4 * j;
    if (!qtr_icp_finite3(t[0], t[1], t[2])) continue;
    g.at[Cells::key((int64_t)g.cell(t[0]), (int64_t)g.cell(t[1]), (int64_t)g.cell(t[2]))].push_back(j);
  }
  if (ns > 0 && !g.at.empty()) st.reason = QTR_ICP_RUNNING;
  const int nchunk = (ns + QTR_ICP_CHUNK - 1) / QTR_ICP_CHUNK;
  std::vector<double> terms((size_t)nchunk * QTR_ICP_CHUNK * QTR_ICP_NT, 0.0);
  for (int eval = 0; st.reason == QTR_ICP_RUNNING; ++eval) {
    std::fill(terms.begin(), terms.end(), 0.0);
    for (int i = 0; i < ns; ++i) {
      const float* p = src4 + 4 * i;
      const float* a = src_nrm4 + 4 * i;
      int best = -1;
      double bd = 0, q[3];
      if (qtr_icp_finite3(p[0], p[1], p[2]) && qtr_icp_normal_ok(a[0], a[1], a[2])) {
        qtr_icp_transform(st.T, p[0], p[1], p[2], q);
        const double f[3] = {g.cell(q[0]), g.cell(q[1]), g.cell(q[2])};
        if (std::fabs(f[0]) < 1e15 && std::fabs(f[1]) < 1e15 && std::fabs(f[2]) < 1e15)  // (also false for NaN)
          for (int64_t dx = -1; dx <= 1; ++dx)
            for (int64_t dy = -1; dy <= 1; ++dy)
              for (int64_t dz = -1; dz <= 1; ++dz) {
                auto it = g.at.find(Cells::key((int64_t)f[0] + dx, (int64_t)f[1] + dy, (int64_t)f[2] + dz));
                if (it == g.at.end()) continue;
                for (int j : it->second) {
                  const float* t = tgt4 + 4 * j;
                  const double d2 = qtr_icp_d2(q, t[0], t[1], t[2]);
                  if (d2 <= cfg.max_d2 && (best < 0 || d2 < bd || (d2 == bd && j < best))) {
                    best = j;
                    bd = d2;
                  }
                }
              }
      }
      if (best >= 0 && !qtr_icp_normal_ok(tgt_nrm4[4 * best], tgt_nrm4[4 * best + 1], tgt_nrm4[4 * best + 2])) best = -1;
      if (corr_at && (eval == corr_iter || corr_iter < 0)) corr_at[i] = best;
      if (best >= 0) {
        const float* t = tgt4 + 4 * best;
        const float* n = tgt_nrm4 + 4 * best;
        qtr_icp_gicp_terms(st.T, q, a[0], a[1], a[2], t[0], t[1], t[2], n[0], n[1], n[2], bd, &terms[(size_t)i * QTR_ICP_NT]);
      }
    }
    double S[QTR_ICP_NT];
    for (int k = 0; k < QTR_ICP_NT; ++k) {
      double acc = 0.0;
      for (int c = 0; c < nchunk; ++c) {
        double w[4];
        for (int wv = 0; wv < 4; ++wv) {
          double p64[64];
          for (int l = 0; l < 64; ++l) p64[l] = terms[((size_t)c * QTR_ICP_CHUNK + wv * 64 + l) * QTR_ICP_NT + k];
          w[wv] = qtr_icp_fold64(p64);
        }
        const double part = qtr_icp_chunk_sum(w);
        acc = (c == 0) ? part : acc + part;
      }
      S[k] = k <= QTR_ICP_T_CNT ? acc : 0.0;
    }
    double* tr = trace ? trace + (size_t)st.iterations * 18 : nullptr;
    qtr_icp_step(&cfg, S, &st, tr);
  }
  for (int k = 0; k < 16; ++k) T_out[k] = st.T[k];
  info[0] = st.iterations;
  info[1] = st.reason;
  info[2] = st.valid;
  info[3] = st.converged;
  info[4] = st.n_corr;
  fit_rmse[0] = st.fitness;
  fit_rmse[1] = st.rmse;
  return 0;
}
