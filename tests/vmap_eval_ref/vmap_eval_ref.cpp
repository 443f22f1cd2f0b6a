// vmap_eval_ref.cpp — host restatement of the evaluation of a pose against the voxel map (quatro_amd/csrc/voxelmap_eval.hip)
// for the tests: the same include/qtr_vmap_eval_math.h arithmetic (qtr_vmap_query, qtr_vmap_eval_terms, the fixed-shape sums,
// qtr_vmap_eval_finish) over a map given by its fetched sections in ascending key order (COORDS, COUNT, SUMS, RECORDS).
// The table is a std::map keyed by the contract's key, so nothing of the device's hashing is restated.  Built by the tests
// with g++ -O2 -ffp-contract=off -shared -fPIC.
#include <cstddef>
#include <cstring>
#include <map>
#include <vector>

#include "qtr_vmap_eval_math.h"
#include "quatro_voxelmap_eval.h"

extern "C" {

// Returns 0; 1 when a voxel's RECORDS row is not qtr_icp_voxel_finish of its SUMS row and COUNT bit for bit (the sections
// do not belong together).  S_out [QTR_VMAP_EVAL_NT], corr_out [n] and point_out [n][2] may be null.
int vmap_eval_ref_run(double side, int nv, const int* coords, const int* count, const double* sums, const double* records,
                      const float* src4, const float* nrm4, int n, const double* T16, QtrVmapEvalRecord* rec, double* S_out,
                      int* corr_out, double* point_out) {
  std::map<unsigned long long, QtrIcpVoxel> vox;
  for (int j = 0; j < nv; ++j) {
    QtrIcpVoxel vx, chk;
    for (int a = 0; a < 3; ++a) vx.mu[a] = records[9 * j + a];
    for (int a = 0; a < 6; ++a) vx.C[a] = records[9 * j + 3 + a];
    vx.n = count[j];
    vx.rep = 0;
    qtr_icp_voxel_finish(sums + 9 * j, count[j], 0, &chk);
    if (memcmp(chk.mu, vx.mu, sizeof(vx.mu)) != 0 || memcmp(chk.C, vx.C, sizeof(vx.C)) != 0) return 1;
    vox[qtr_vmap_key(coords[3 * j], coords[3 * j + 1], coords[3 * j + 2])] = vx;
  }
  double T[16];
  for (int k = 0; k < 16; ++k) T[k] = k < 12 ? T16[k] : (k == 15 ? 1.0 : 0.0);  // (row 3 is taken as 0 0 0 1)
  const int nchunk = (n + QTR_ICP_CHUNK - 1) / QTR_ICP_CHUNK;
  std::vector<double> terms((size_t)nchunk * QTR_ICP_CHUNK * QTR_VMAP_EVAL_NT, 0.0);
  for (int i = 0; i < n; ++i) {
    const float* p = src4 + 4 * i;
    const float* a = nrm4 + 4 * i;
    double* e = &terms[(size_t)i * QTR_VMAP_EVAL_NT];
    int best = -1;
    if (qtr_icp_finite3(p[0], p[1], p[2])) {
      double q[3] = {0.0, 0.0, 0.0};
      unsigned long long key = 0;
      const QtrIcpVoxel* hit = nullptr;
      if (qtr_vmap_query(T, p[0], p[1], p[2], a[0], a[1], a[2], side, q, &key)) {
        auto it = vox.find(key);
        if (it != vox.end() && it->second.n > 0) hit = &it->second;
      }
      qtr_vmap_eval_terms(T, q, a[0], a[1], a[2], hit, e);
      best = hit ? 0 : -1;
    }
    if (corr_out) corr_out[i] = best;
    if (point_out) {
      point_out[2 * i] = e[QTR_ICP_T_R2];
      point_out[2 * i + 1] = e[QTR_ICP_T_W];
    }
  }
  double S[QTR_VMAP_EVAL_NT];
  for (int k = 0; k < QTR_VMAP_EVAL_NT; ++k) {
    double acc = 0.0;
    for (int c = 0; c < nchunk; ++c) {
      double w[4];
      for (int wv = 0; wv < 4; ++wv) {
        double p64[64];
        for (int l = 0; l < 64; ++l) p64[l] = terms[((size_t)c * QTR_ICP_CHUNK + wv * 64 + l) * QTR_VMAP_EVAL_NT + k];
        w[wv] = qtr_icp_fold64(p64);
      }
      const double part = qtr_icp_chunk_sum(w);
      acc = (c == 0) ? part : acc + part;
    }
    S[k] = acc;
  }
  if (S_out) memcpy(S_out, S, sizeof(S));
  qtr_vmap_eval_finish(S, rec);
  return 0;
}

void vmap_eval_ref_finish(const double* S, QtrVmapEvalRecord* rec) { qtr_vmap_eval_finish(S, rec); }
int vmap_eval_ref_best(const QtrVmapEvalRecord* r, int B) { return qtr_vmap_eval_best(r, B); }

// sizes, offsets and constants for the ctypes mirrors
void vmap_eval_ref_layout(int* out) {
  out[0] = (int)sizeof(QtrVmapEvalRecord);
  out[1] = (int)sizeof(qtr_vmap_eval_result);
  out[2] = (int)sizeof(qtr_vmap_eval_params);
  out[3] = (int)offsetof(qtr_vmap_eval_result, status);
  out[4] = (int)offsetof(qtr_vmap_eval_result, valid);
  out[5] = (int)offsetof(qtr_vmap_eval_result, n_source);
  out[6] = (int)offsetof(qtr_vmap_eval_result, n_corr);
  out[7] = (int)offsetof(qtr_vmap_eval_result, overlap);
  out[8] = (int)offsetof(qtr_vmap_eval_result, sum_d2);
  out[9] = (int)offsetof(qtr_vmap_eval_result, inlier_rmse);
  out[10] = (int)offsetof(qtr_vmap_eval_result, sum_w);
  out[11] = (int)offsetof(qtr_vmap_eval_result, chi2);
  out[12] = (int)offsetof(qtr_vmap_eval_result, rmse);
  out[13] = (int)offsetof(qtr_vmap_eval_result, information);
  out[14] = (int)offsetof(qtr_vmap_eval_result, hessian);
  out[15] = (int)offsetof(qtr_vmap_eval_result, gradient);
  out[16] = (int)offsetof(qtr_vmap_eval_params, per_point);
  out[17] = QTR_VMAP_EVAL_MAX;
  out[18] = QTR_VMAP_EVAL_CORR;
  out[19] = QTR_VMAP_EVAL_POINT;
  out[20] = QTR_VMAP_EVAL_TIMES;
  out[21] = QTR_VMAP_EVAL_NT;
  out[22] = (int)offsetof(QtrVmapEvalRecord, overlap);
  out[23] = (int)offsetof(QtrVmapEvalRecord, information);
}
}
