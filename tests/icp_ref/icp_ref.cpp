// icp_ref.cpp — host restatement of the device ICP loop (quatro_amd/csrc/icp.hip) for the tests: the same
// include/qtr_icp_math.h arithmetic, the same fixed-shape sums, a plain hash grid for the nearest-neighbour search
// (the search's result does not depend on the grid: nearest binary64 d^2, ties to the lowest target index).
// Built by the tests with g++ -O2 -ffp-contract=off -shared -fPIC.
#include <cmath>
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "qtr_icp_math.h"

namespace {
struct Grid {
  double mn[3] = {0, 0, 0}, cell = 1;
  // (three whole indices per key: a packed key wraps where a query lies millions of cells from the box)
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
  std::unordered_map<Key, std::vector<int>, Hash> cells;
  static Key key(int64_t x, int64_t y, int64_t z) { return Key{x, y, z}; }
};
}  // namespace

extern "C" int icp_ref_run(const float* src4, int ns, const float* tgt4, int nt, const float* nrm4, const double* guess,
                           double max_d, double teps, double feps, int max_iter, int method, int min_corr,
                           double* T_out, int* info /* iterations, reason, valid, converged, n_corr */,
                           double* fit_rmse /* 2 */, double* trace /* max_iter x 18 */,
                           int* corr_at /* ns or null */, int corr_iter /* evaluation whose correspondences to keep */) {
  QtrIcpCfg cfg;
  cfg.max_d2 = max_d * max_d;
  cfg.trans_eps = teps;
  cfg.fit_eps = feps;
  cfg.max_iterations = max_iter;
  cfg.method = method;
  cfg.min_corr = min_corr > 0 ? min_corr : (method == 0 ? 6 : 3);
  cfg.pad = 0;
  QtrIcpState st;
  qtr_icp_init(&st, guess);
  st.reason = QTR_ICP_STOP_TOO_FEW;
  Grid g;
  bool any = false;
  for (int j = 0; j < nt; ++j) {
    const float* t = tgt4 + 4 * j;
    if (!qtr_icp_finite3(t[0], t[1], t[2])) continue;
    for (int a = 0; a < 3; ++a) g.mn[a] = any ? std::fmin(g.mn[a], (double)t[a]) : (double)t[a];
    any = true;
  }
  if (ns > 0 && any) {
    st.reason = QTR_ICP_RUNNING;
    g.cell = max_d * 1.001;
    for (int j = 0; j < nt; ++j) {
      const float* t = tgt4 + 4 * j;
      if (!qtr_icp_finite3(t[0], t[1], t[2])) continue;
      int64_t c[3];
      for (int a = 0; a < 3; ++a) c[a] = (int64_t)std::floor(((double)t[a] - g.mn[a]) / g.cell);
      g.cells[Grid::key(c[0], c[1], c[2])].push_back(j);
    }
  }
  const int nchunk = (ns + QTR_ICP_CHUNK - 1) / QTR_ICP_CHUNK;
  std::vector<double> terms((size_t)nchunk * QTR_ICP_CHUNK * QTR_ICP_NT, 0.0);
  for (int eval = 0; st.reason == QTR_ICP_RUNNING; ++eval) {
    std::fill(terms.begin(), terms.end(), 0.0);
    for (int i = 0; i < ns; ++i) {
      const float* p = src4 + 4 * i;
      int best = -1;
      double bd = 0, q[3];
      if (qtr_icp_finite3(p[0], p[1], p[2])) {
        qtr_icp_transform(st.T, p[0], p[1], p[2], q);
        double f[3];
        bool in = true;
        for (int a = 0; a < 3; ++a) {
          f[a] = std::floor((q[a] - g.mn[a]) / g.cell);
          if (!(std::fabs(f[a]) < 1e15)) in = false;
        }
        if (in)
          for (int64_t dz = -1; dz <= 1; ++dz)
            for (int64_t dy = -1; dy <= 1; ++dy)
              for (int64_t dx = -1; dx <= 1; ++dx) {
                auto it = g.cells.find(Grid::key((int64_t)f[0] + dx, (int64_t)f[1] + dy, (int64_t)f[2] + dz));
                if (it == g.cells.end()) continue;
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
      if (best >= 0 && method == 0 && !qtr_icp_finite3(nrm4[4 * best], nrm4[4 * best + 1], nrm4[4 * best + 2])) best = -1;
      if (corr_at && (eval == corr_iter || corr_iter < 0)) corr_at[i] = best;
      if (best >= 0) {
        const float* t = tgt4 + 4 * best;
        const float* n = method == 0 ? nrm4 + 4 * best : nullptr;
        qtr_icp_terms(method, q, t[0], t[1], t[2], n ? n[0] : 0.f, n ? n[1] : 0.f, n ? n[2] : 0.f, bd,
                      &terms[(size_t)i * QTR_ICP_NT]);
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
