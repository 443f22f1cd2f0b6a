// vmap_ct_ref.cpp — host restatement of the continuous-time registration against the voxel map
// (quatro_amd/csrc/voxelmap_ct.hip) for the tests: the same include/qtr_vmap_ct_math.h arithmetic and the same fixed-shape
// sums as the device iteration.  The map arrives as the finished records a RefMap of tests/vmap_restate.py fetches (voxel
// coordinates, member counts, mu and C_b), so nothing of that restatement is repeated here.
// Built by the tests with g++ -O2 -ffp-contract=off -shared -fPIC.
#include <algorithm>
#include <cstddef>
#include <cstring>
#include <map>
#include <vector>

#include "qtr_vmap_ct_math.h"
#include "quatro_voxelmap_ct.h"

namespace {
const double kIdentity[16] = {1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
}

extern "C" {

// sizeof and the three offsets of qtr_vmap_ct_info
void vmap_ct_ref_layout(int* out) {
  out[0] = (int)sizeof(qtr_vmap_ct_info);
  out[1] = (int)offsetof(qtr_vmap_ct_info, n_points);
  out[2] = (int)offsetof(qtr_vmap_ct_info, n_skipped);
  out[3] = (int)offsetof(qtr_vmap_ct_info, n_extrapolated);
}

// 1 and T16 (row 3 = 0 0 0 1): the pose at t; 0: the interval is refused
int vmap_ct_ref_pose_at(double t_begin, double t_end, const double* B, const double* E, double t, double* T16) {
  if (!qtr_vmap_ct_pose_at(t_begin, t_end, B, E, t, T16)) return 0;
  T16[12] = T16[13] = T16[14] = 0.0;
  T16[15] = 1.0;
  return 1;
}

// One point under the iterate E.  iv20: the interval as 20 doubles (tau, div, R, c, dc, w).  out: [0] interval admitted,
// [1] the census's flags, [2] qtr_vmap_ct_query's verdict, [3 .. 14] T = [R(u) | c(u)], [15 .. 17] q, [18 .. 20] r, [21] s,
// [22 .. 53] the terms against the record rec9 (mu 3, C_b 6) with n_members members (zeros without a verdict or a record).
void vmap_ct_ref_point(double t_begin, double t_end, const double* B, const double* E, const float* p4, const float* a4, float time,
                       double side, const double* rec9, int n_members, double* iv20, double* out, unsigned long long* key) {
  QtrDeskewInterval iv;
  for (int k = 0; k < 54; ++k) out[k] = 0.0;
  *key = 0;
  out[0] = qtr_vmap_ct_interval(t_begin, t_end, B, E, &iv) ? 1.0 : 0.0;
  memcpy(iv20, &iv, sizeof(iv));
  out[1] = (double)qtr_vmap_ct_flags(t_end, t_begin - t_end, p4[0], p4[1], p4[2], a4[0], a4[1], a4[2], time);
  if (out[0] == 0.0) return;
  double s = 0.0;
  const bool ok = qtr_vmap_ct_query(&iv, p4[0], p4[1], p4[2], a4[0], a4[1], a4[2], time, side, out + 3, out + 15, out + 18, &s, key);
  out[2] = ok ? 1.0 : 0.0;
  out[21] = s;
  if (!ok || !rec9) return;
  QtrIcpVoxel vx;
  for (int a = 0; a < 3; ++a) vx.mu[a] = rec9[a];
  for (int a = 0; a < 6; ++a) vx.C[a] = rec9[3 + a];
  vx.n = n_members;
  vx.rep = 0;
  qtr_vmap_ct_terms(out + 3, out + 15, out + 18, s, a4[0], a4[1], a4[2], &vx, out + 22);
}

// The registration loop: vmap_ref_register's (tests/vmap_ref/vmap_ref.cpp) with the interval of the current E in front of every
// evaluation and the continuous-time terms.  The map: nv voxels by coordinates, member counts and finished records.
// corr_at (ns or null): 0 matched / -1 none at evaluation corr_iter (< 0: the last one evaluated).  ct_info: n_points,
// n_skipped, n_extrapolated.
void vmap_ct_ref_register(const int* coords, const int* count, const double* records, int nv, double side, const float* src4, int ns,
                          const float* src_nrm4, const float* times, double t_begin, double t_end, const double* begin_pose,
                          const double* guess, double teps, double feps, int max_iter, int min_corr, double* T_out,
                          int* info /* iterations, reason, valid, converged, n_corr */, double* fit_rmse /* 2 */,
                          double* trace /* max_iter x 18 */, int* corr_at, int corr_iter, int* ct_info) {
  std::map<unsigned long long, QtrIcpVoxel> rec;
  for (int j = 0; j < nv; ++j) {
    QtrIcpVoxel vx;
    for (int a = 0; a < 3; ++a) vx.mu[a] = records[9 * j + a];
    for (int a = 0; a < 6; ++a) vx.C[a] = records[9 * j + 3 + a];
    vx.n = count[j];
    vx.rep = 0;
    rec[qtr_vmap_key(coords[3 * j], coords[3 * j + 1], coords[3 * j + 2])] = vx;
  }
  ct_info[0] = ns;
  ct_info[1] = ct_info[2] = 0;
  for (int i = 0; i < ns; ++i) {
    const int f = qtr_vmap_ct_flags(t_end, t_begin - t_end, src4[4 * i], src4[4 * i + 1], src4[4 * i + 2], src_nrm4[4 * i],
                                    src_nrm4[4 * i + 1], src_nrm4[4 * i + 2], times[i]);
    ct_info[1] += f == QTR_VMAP_CT_SKIPPED ? 1 : 0;
    ct_info[2] += f == QTR_VMAP_CT_EXTRAPOLATED ? 1 : 0;
  }
  QtrIcpCfg cfg;
  cfg.max_d2 = side * side;
  cfg.trans_eps = teps;
  cfg.fit_eps = feps;
  cfg.max_iterations = max_iter;
  cfg.method = 3;
  cfg.min_corr = min_corr > 0 ? min_corr : 4;
  cfg.pad = 0;
  double g[16];
  for (int k = 0; k < 16; ++k) g[k] = k < 12 ? guess[k] : kIdentity[k];  // (row 3 is taken as 0 0 0 1)
  QtrIcpState st;
  qtr_icp_init(&st, g);
  st.reason = ns > 0 ? QTR_ICP_RUNNING : QTR_ICP_STOP_TOO_FEW;
  const int nchunk = (ns + QTR_ICP_CHUNK - 1) / QTR_ICP_CHUNK;
  std::vector<double> terms((size_t)nchunk * QTR_ICP_CHUNK * QTR_ICP_NT, 0.0);
  for (int eval = 0; st.reason == QTR_ICP_RUNNING; ++eval) {
    std::fill(terms.begin(), terms.end(), 0.0);
    QtrDeskewInterval iv;
    const bool admitted = qtr_vmap_ct_interval(t_begin, t_end, begin_pose, st.T, &iv);
    for (int i = 0; i < ns; ++i) {
      const float* p = src4 + 4 * i;
      const float* a = src_nrm4 + 4 * i;
      int best = -1;
      double T[12], q[3], r[3], s = 0.0;
      unsigned long long key = 0;
      if (admitted && qtr_vmap_ct_query(&iv, p[0], p[1], p[2], a[0], a[1], a[2], times[i], side, T, q, r, &s, &key)) {
        auto it = rec.find(key);
        if (it != rec.end() && it->second.n > 0) {
          best = 0;
          qtr_vmap_ct_terms(T, q, r, s, a[0], a[1], a[2], &it->second, &terms[(size_t)i * QTR_ICP_NT]);
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
}

}  // extern "C"
