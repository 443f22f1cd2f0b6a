// vgicp_ref.cpp — host restatement of the device loop's voxelised plane-to-plane method (quatro_amd/csrc/icp.hip,
// k_icp_voxel_stats and d_icp_iter<3>) for the tests: the same include/qtr_icp_math.h arithmetic (the grid rule, the
// voxel records, qtr_icp_vgicp_terms, qtr_icp_step) and the same fixed-shape sums.  Unlike the search methods' the grid is
// part of the contract, so nothing here is the restatement's own.  Built by the tests with g++ -O2 -ffp-contract=off
// -shared -fPIC.
#include <algorithm>
#include <cmath>
#include <unordered_map>
#include <vector>

#include "qtr_icp_math.h"

// feed (nt indices or null): the order in which the targets are handed to their cells — the records must not depend on it.
// rec_out (nt x 11 or null): for the representative j of every voxel [N, mu (3), C_b (6), cell]; zero elsewhere.
// Returns 0, or -1 when the grid exceeds QTR_ICP_CELL_CAP cells (ncell_out then holds the count the rule gives).
extern "C" int vgicp_ref_run(const float* src4, int ns, const float* src_nrm4, const float* tgt4, int nt, const float* tgt_nrm4,
                             const int* feed, const double* guess, double side, double teps, double feps, int max_iter,
                             int min_corr, double* T_out, int* info /* iterations, reason, valid, converged, n_corr */,
                             double* fit_rmse /* 2 */, double* trace /* max_iter x 18 */, int* corr_at /* ns or null */,
                             int corr_iter, double* rec_out, double* grid_out /* o (3), dims (3), cells */) {
  QtrIcpCfg cfg;
  cfg.max_d2 = side * side;
  cfg.trans_eps = teps;
  cfg.fit_eps = feps;
  cfg.max_iterations = max_iter;
  cfg.method = 3;
  cfg.min_corr = min_corr > 0 ? min_corr : 4;
  cfg.pad = 0;
  QtrIcpState st;
  qtr_icp_init(&st, guess);
  st.reason = QTR_ICP_STOP_TOO_FEW;
  for (int k = 0; k < 16; ++k) T_out[k] = st.T[k];
  for (int k = 0; k < 5; ++k) info[k] = 0;
  info[1] = st.reason;
  fit_rmse[0] = st.fitness;
  fit_rmse[1] = st.rmse;
  // the box of the finite target points (float minima / maxima, as the device's atomics take them)
  bool any = false;
  float lo[3] = {0, 0, 0}, hi[3] = {0, 0, 0};
  for (int j = 0; j < nt; ++j) {
    const float* t = tgt4 + 4 * j;
    if (!qtr_icp_finite3(t[0], t[1], t[2])) continue;
    for (int a = 0; a < 3; ++a) {
      lo[a] = (!any || t[a] < lo[a]) ? t[a] : lo[a];
      hi[a] = (!any || t[a] > hi[a]) ? t[a] : hi[a];
    }
    any = true;
  }
  double o[3] = {0, 0, 0}, mx[3] = {0, 0, 0};
  int dims[3] = {0, 0, 0};
  std::unordered_map<int, std::vector<int>> cells;
  std::unordered_map<int, QtrIcpVoxel> vox;
  if (any && ns > 0) {
    for (int a = 0; a < 3; ++a) {
      o[a] = (double)lo[a];
      mx[a] = (double)hi[a];
    }
    const double nc = qtr_icp_voxel_dims(o, mx, side, dims);
    if (grid_out) {
      for (int a = 0; a < 3; ++a) {
        grid_out[a] = o[a];
        grid_out[3 + a] = (double)dims[a];
      }
      grid_out[6] = nc;
    }
    if (!(nc <= (double)QTR_ICP_CELL_CAP)) return -1;
    for (int f = 0; f < nt; ++f) {
      const int j = feed ? feed[f] : f;
      const float* t = tgt4 + 4 * j;
      const float* b = tgt_nrm4 + 4 * j;
      if (!qtr_icp_finite3(t[0], t[1], t[2]) || !qtr_icp_normal_ok(b[0], b[1], b[2])) continue;
      const double q[3] = {(double)t[0], (double)t[1], (double)t[2]};
      int lin = 0;
      if (qtr_icp_voxel_cell(q, o, side, dims, &lin)) cells[lin].push_back(j);  // (always inside: the box is the targets')
    }
    for (auto& kv : cells) {
      std::vector<int>& m = kv.second;
      std::sort(m.begin(), m.end());  // the contract's order: ascending original index
      double acc[9] = {0, 0, 0, 0, 0, 0, 0, 0, 0};
      for (int j : m)
        qtr_icp_voxel_add(acc, tgt4[4 * j], tgt4[4 * j + 1], tgt4[4 * j + 2], tgt_nrm4[4 * j], tgt_nrm4[4 * j + 1],
                          tgt_nrm4[4 * j + 2]);
      QtrIcpVoxel vx;
      qtr_icp_voxel_finish(acc, (int)m.size(), m[0], &vx);
      vox[kv.first] = vx;
      if (rec_out) {
        double* r = rec_out + (size_t)11 * m[0];
        r[0] = (double)vx.n;
        for (int a = 0; a < 3; ++a) r[1 + a] = vx.mu[a];
        for (int a = 0; a < 6; ++a) r[4 + a] = vx.C[a];
        r[10] = (double)kv.first;
      }
    }
    st.reason = QTR_ICP_RUNNING;
  }
  const int nchunk = (ns + QTR_ICP_CHUNK - 1) / QTR_ICP_CHUNK;
  std::vector<double> terms((size_t)nchunk * QTR_ICP_CHUNK * QTR_ICP_NT, 0.0);
  for (int eval = 0; st.reason == QTR_ICP_RUNNING; ++eval) {
    std::fill(terms.begin(), terms.end(), 0.0);
    for (int i = 0; i < ns; ++i) {
      const float* p = src4 + 4 * i;
      const float* a = src_nrm4 + 4 * i;
      int best = -1;
      if (qtr_icp_finite3(p[0], p[1], p[2]) && qtr_icp_normal_ok(a[0], a[1], a[2])) {
        double q[3];
        qtr_icp_transform(st.T, p[0], p[1], p[2], q);
        int lin = 0;
        if (qtr_icp_voxel_cell(q, o, side, dims, &lin)) {
          auto it = vox.find(lin);
          if (it != vox.end()) {
            best = it->second.rep;
            qtr_icp_vgicp_terms(st.T, q, a[0], a[1], a[2], &it->second, &terms[(size_t)i * QTR_ICP_NT]);
          }
        }
      }
      if (corr_at && (eval == corr_iter || corr_iter < 0)) corr_at[i] = best;
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
      S[k] = k <= QTR_ICP_T_W ? acc : 0.0;
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
